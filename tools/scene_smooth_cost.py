"""What scene_smooth.smooth_scene costs on a furnished room of about 1 M points, span by span, beside a torch formulation of
the sweeps (index_add_ over an edge list) and, at a smaller size, the numpy restatement.

    python tools/scene_smooth_cost.py [--points 1000000] [--calls 9] [--voxel 0.05] [--iterations 10] [--check-points 100000]
                                      [--scan room|volume] [--cols 3]

--scan room (the default): synthetic.make_room(seed=0, n_points, extent=(8, 6, 3)), a floor (class 0), four walls (class 1)
and three boxes (class 2): surfaces, many points a voxel.  --scan volume: synthetic.make_scene, the same extent filled with
uniform points, three slabs along x as classes -- about 1.5 points per occupied voxel at 0.05 m, so the voxel graph is as
large as the scan allows (the scan of profiles/r22_scene_grow.md).  The result to smooth is built by hand, --cols columns
(3): logits +1 for the class a point shows and -1 for the others, times 1 .. 3 votes; 15 % of the points show a wrong class
(one of the first three) and 10 % have no vote.  Per connectivity (26, the default, and 6), by
the method of tools/scene_grow_cost.py: after a warm-up call, `calls` calls each between one HIP event pair (the call's
three host reads lie inside it) and the host clock, reported as median, minimum and maximum; then `calls` more with event
pairs THIS TOOL puts around the ops wrappers -- bounds, sort, voxels, evidence, graph, sweep (all `iterations` launches),
spread -- and the host clock around the record reads.  From the spans: the time of one sweep, the bytes it must move (the
neighbour table, Z in and Z out) and what it reads at the least (the packed slots in use, one ring and one row per edge
aside), and the bytes per second that makes; the graph launch is one walk over the 27 cells with its binary searches, what a
sweep without the table would pay again every time.  The torch formulation runs the same sweeps from the same evidence and
neighbour table: gathers, two index_add_ (float atomics: not the same bits) and a where per sweep.  --check-points: the
numpy restatement tests/scene_smooth_ref.py on a room of that many points, every field against the device (0: skip).
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from scene_grow_cost import stats, timed_calls  # noqa: E402
from scene_objects_cost import spans  # noqa: E402

from r3dfsseg_amd import ops, scene, scene_grow as G, scene_smooth as SM, synthetic as S  # noqa: E402

SPANS = {"scene_grow_bounds": "bounds", "scene_grow_sort": "sort", "scene_grow_voxels": "voxels", "scene_smooth_evidence": "evidence",
         "scene_smooth_graph": "graph", "scene_smooth_sweep": "sweep", "scene_smooth_spread": "spread"}
N_CLASSES = 3


def labelled_room(n_points, seed=0, kind="room", cols=3):
    """-> (scan (M, 6) fp32 on the host, scores (M, cols) fp32, votes (M,) int32, labels (M,) int64, truth (M,) int64)."""
    if kind == "room":
        import scene_objects_cases as OC
        scan, surface = S.make_room(seed=seed, n_points=n_points, extent=(8.0, 6.0, 3.0))
        truth = OC.labels_of_surface(surface.numpy()).astype(np.int64)
    else:
        scan = S.make_scene(S.workload_cfg("S"), seed=seed, extent=(8.0, 6.0, 3.0), n_points=n_points)[0][:, :6].contiguous()
        x = scan[:, 0].numpy()
        truth = np.clip(np.floor(3.0 * (x - x.min()) / (x.max() - x.min())), 0, 2).astype(np.int64)
    rs = np.random.RandomState(seed + 1)
    M = len(truth)
    shown = np.where(rs.rand(M) < 0.15, (truth + rs.randint(1, N_CLASSES, M)) % N_CLASSES, truth)
    votes = rs.randint(1, 4, M).astype(np.int32)
    votes[rs.rand(M) < 0.10] = 0
    scores = np.where(shown[:, None] == np.arange(cols)[None, :], 1.0, -1.0).astype(np.float32) * votes[:, None].astype(np.float32)
    labels = np.where(votes > 0, shown, -1).astype(np.int64)
    return scan, scores, votes, labels, truth


def result_of(scores, votes, labels):
    return scene.SceneResult(labels=torch.from_numpy(labels).cuda(), scores=torch.from_numpy(scores).cuda(),
                             votes=torch.from_numpy(votes).cuda(), n_blocks=0, n_chunks=0, n_unlabelled=int((labels == -1).sum()),
                             redone=0)


def torch_sweeps(evidence, members, nbr, alpha, iterations):
    """S4 in torch from the device's evidence and neighbour table -> (Z, ring).  index_add_ adds floats by atomics."""
    V, C = evidence.shape
    v_idx = torch.arange(V, device=nbr.device).repeat(nbr.shape[0])
    u_idx = nbr.reshape(-1).long()
    on = u_idx >= 0
    v_idx, u_idx = v_idx[on], u_idx[on]
    a = torch.tensor(alpha, dtype=torch.float32, device=nbr.device)
    b = 1 - a
    member = members > 0
    Z, ring = evidence.clone(), torch.where(member, 0, -1).int()
    for t in range(iterations):
        live = ((ring >= 0) & (ring <= t))[u_idx]
        s = torch.zeros_like(Z).index_add_(0, v_idx[live], Z[u_idx[live]])
        n = torch.zeros(V, device=Z.device).index_add_(0, v_idx[live], torch.ones(int(live.sum()), device=Z.device))
        m = s / n.clamp(min=1)[:, None]
        has = n > 0
        Z = torch.where((has & member)[:, None], b * evidence + a * m, torch.where((has & ~member)[:, None], m, Z))
        ring = torch.where(has & ~member & (ring < 0), t + 1, ring)
    return Z, ring


def sweep_traffic(sm, nbr, iterations, sweep_ms):
    V, C = sm.voxel_scores.shape
    edges = int((nbr >= 0).sum())
    per_sweep_us = sweep_ms / max(iterations, 1) * 1e3
    must = 4 * (nbr.numel() + 2 * V * C)
    # what a sweep reads at the least: per voxel its slots in use and the first empty one, its own ring; per edge the
    # neighbour's ring and row; Y for a member voxel; Z out
    least = 4 * (edges + V + V + edges + edges * C + V * C + V * C)
    return {"edges": edges, "mean_degree": round(edges / V, 2), "per_sweep_us": round(per_sweep_us, 2),
            "bytes_table_plus_z_in_out": must, "gb_per_s_table_plus_z": round(must / per_sweep_us / 1e3, 1),
            "bytes_touched_at_least": least, "gb_per_s_touched": round(least / per_sweep_us / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--check-points", type=int, default=100000)
    ap.add_argument("--scan", choices=("room", "volume"), default="room")
    ap.add_argument("--cols", type=int, default=3)
    args = ap.parse_args()
    assert 3 <= args.cols <= 64
    scan_host, scores, votes, labels, truth = labelled_room(args.points, kind=args.scan, cols=args.cols)
    scan, res = scan_host.cuda(), result_of(scores, votes, labels)
    out = {"points": args.points, "calls": args.calls, "voxel": args.voxel, "iterations": args.iterations, "scan": args.scan, "cols": args.cols, "runs": []}
    for conn in (26, 6):
        smooth = lambda: SM.smooth_scene(res, scan, voxel=args.voxel, connectivity=conn, iterations=args.iterations)
        rec = {"connectivity": conn, "smooth_scene": timed_calls(smooth, args.calls),
               "span_ms": spans(smooth, args.calls, SPANS, G)}
        sm = smooth()
        # the neighbour table is no field of the result: built again, as the call builds it
        ws = ops.scene_grow_workspace(len(scan), scan.device)
        ops.scene_grow_bounds(scan, ws)
        r = G.read_record(ws)
        lo, hi = G.extent_of(r)
        ops.scene_grow_sort(scan, lo, np.float32(args.voxel), sm.grid, ws)
        ops.scene_grow_voxels(scan, sm.grid, r[ops.GROW_R_NVALID], sm.n_voxels, False, ws)
        nbr = ops.scene_smooth_graph(len(scan), sm.grid, sm.n_voxels, conn, None, None, ws)
        rec["sweep"] = sweep_traffic(sm, nbr, args.iterations, rec["span_ms"]["sweep"]["median"])
        rec["walk_us"] = round(rec["span_ms"]["graph"]["median"] * 1e3, 2)
        torch_run = lambda: torch_sweeps(sm.voxel_evidence, sm.voxel_members, nbr, 0.8, args.iterations)
        rec["torch_sweeps"] = timed_calls(torch_run, args.calls)
        Zt, ring_t = torch_run()
        rec["torch_max_abs_diff"] = float((Zt - sm.voxel_scores).abs().max())
        rec["torch_ring_equal"] = bool(torch.equal(ring_t, sm.voxel_ring))
        wrong = lambda lab: int((lab.cpu().numpy() != truth).sum())
        rec.update(grid=list(sm.grid), n_voxels=sm.n_voxels, n_member_voxels=sm.n_member_voxels, n_filled_voxels=sm.n_filled_voxels,
                   n_smoothed=sm.n_smoothed, n_changed=sm.n_changed, n_filled=sm.n_filled, n_unlabelled=sm.n_unlabelled,
                   wrong_points_before=wrong(res.labels), wrong_points_after=wrong(sm.labels))
        out["runs"].append(rec)
        print("connectivity %d: done" % conn, file=sys.stderr, flush=True)
    if args.check_points > 0:
        import scene_smooth_ref as R
        scan_c, scores_c, votes_c, labels_c, _ = labelled_room(args.check_points, kind=args.scan, cols=args.cols)
        got = SM.smooth_scene(result_of(scores_c, votes_c, labels_c), scan_c.cuda(), voxel=args.voxel, iterations=args.iterations)
        t0 = time.perf_counter()
        want = R.smooth(scan_c.numpy(), scores_c, votes_c, labels_c, voxel=args.voxel, iterations=args.iterations)
        same = all(np.array_equal(getattr(got, k).cpu().numpy().view(np.uint32), want[k].view(np.uint32))
                   for k in ("scores", "voxel_scores", "voxel_evidence"))
        same = same and all(np.array_equal(getattr(got, k).cpu().numpy(), want[k]) for k in
                            ("labels", "votes", "smoothed", "voxel_index", "voxel_labels", "voxel_members", "voxel_ring"))
        same = same and all(getattr(got, k) == want[k] for k in ("n_voxels", "n_member_voxels", "n_filled_voxels", "n_smoothed",
                                                                 "n_changed", "n_filled", "n_unlabelled", "n_invalid", "grid"))
        out["restatement"] = {"points": args.check_points, "n_voxels": got.n_voxels, "host_s": round(time.perf_counter() - t0, 2),
                              "equals_device": bool(same)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
