"""What scene_grow.build_segments costs on a scan of about 1 M points, span by span, beside the predict_scene and pool_segments
calls it sits between and beside the numpy restatement on the CPU (the only baseline there is without a region-growing
library).

    python tools/scene_grow_cost.py [--points 1000000] [--calls 7] [--voxel 0.05] [--colour-tol 64] [--baseline one]
                                    [--scan scene|room] [--normal-tol DEGREES] [--min-points N --absorb R [R ...]]

--scan scene (the default): the seeded room of synthetic.make_scene, 8 m x 6 m x 3 m of uniform points with colours in
0 .. 255 -- about one point per occupied voxel at 0.05 m, so the voxel graph is as large as the scan allows.  --scan room:
synthetic.make_room, the same extent as SURFACES (a floor, four walls, three boxes) with 3 mm of noise: fewer voxels with
more points, the scan normal_tol is meant for.  Configurations: connectivity 6 and 26, without colour and with colour_tol;
and both with colour_tol = 0, which joins next to nothing on the uniform scan: the union span is then the neighbour searches
alone, and what the other configurations take beyond it is the hooking.  With --normal-tol the first four are run once
more with that normal_tol, and their spans include the two launches it adds, centroids and normals.  With --absorb (needs
--normal-tol) connectivity 6 and 26 are run with that normal_tol and --min-points once more per ring count, 0 first: the
absorb span (the start launch, one launch per ring, the end launch) and the share of the scan's points that are -1.

Per configuration, after a warm-up call: `calls` calls each timed with one HIP event pair (the call's four host reads lie
inside it) and with the host clock, reported as median, minimum and maximum; then `calls` more with event pairs THIS TOOL
puts around the ops wrappers -- bounds, sort (keys, radix sort, heads, scan), voxels (table and mean colours), centroids
and normals (with normal_tol), union, flatten (roots, counts, kept flags, scan), ids -- and the host clock around the record reads (a read waits for what is
queued in front of it, so it is at least that device time); the medians per span.  predict_scene (ProtoLearner, workload S)
and pool_segments (on the grown segments) are timed the same way on the same scan.  --baseline one | all | none: the numpy
restatement tests/scene_grow_ref.py on the host clock for the first configuration, or for all four, and the check that the
device's segments equal it.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from r3dfsseg_amd import ops, scene_grow as G, scene_segments as SS, synthetic as S  # noqa: E402

SPANS = {"scene_grow_bounds": "bounds", "scene_grow_sort": "sort", "scene_grow_voxels": "voxels",
         "scene_grow_centroids": "centroids", "scene_grow_normals": "normals", "scene_grow_union": "union",
         "scene_grow_union_normals": "union", "scene_grow_components": "flatten", "scene_grow_absorb": "absorb",
         "scene_grow_ids": "ids"}


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed_calls(fn, calls):
    fn()
    torch.cuda.synchronize()
    dev, host = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(a.elapsed_time(b))
    return {"event_ms": stats(dev), "host_ms": stats(host)}


def spans(fn, calls):
    """`calls` calls with event pairs around the ops wrappers and the host clock around the record reads -> medians."""
    orig = {n: getattr(ops, n) for n in SPANS if hasattr(ops, n)}
    read = G.read_record
    runs, reads = [], []

    def wrap(span, f, events):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f(*a, **k)
            e1.record()
            events.append((span, e0, e1))
            return out
        return timed

    for _ in range(calls):
        events, this_reads = [], []

        def timed_read(ws):
            t0 = time.perf_counter()
            out = read(ws)
            this_reads.append((time.perf_counter() - t0) * 1e3)
            return out
        try:
            for n, f in orig.items():
                setattr(ops, n, wrap(SPANS[n], f, events))
            G.read_record = timed_read
            fn()
            torch.cuda.synchronize()
        finally:
            for n, f in orig.items():
                setattr(ops, n, f)
            G.read_record = read
        runs.append({span: e0.elapsed_time(e1) for span, e0, e1 in events})
        reads.append(this_reads)
    out = {span: stats([r[span] for r in runs]) for span in dict.fromkeys(SPANS.values()) if span in runs[0]}
    out["host_reads_median"] = [round(float(np.median([r[i] for r in reads])), 4) for i in range(len(reads[0]))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--colour-tol", type=float, default=64.0)
    ap.add_argument("--baseline", choices=["none", "one", "all"], default="one")
    ap.add_argument("--scan", choices=["scene", "room"], default="scene")
    ap.add_argument("--normal-tol", type=float, default=None)
    ap.add_argument("--min-points", type=int, default=1)
    ap.add_argument("--absorb", type=int, nargs="*", default=[])
    args = ap.parse_args()
    if args.absorb and args.normal_tol is None:
        ap.error("--absorb needs --normal-tol")
    from r3dfsseg_amd.proto_learner import ProtoLearner
    cfg = S.workload_cfg("S")
    if args.scan == "room":
        scan_host = S.make_room(seed=0, n_points=args.points, extent=(8.0, 6.0, 3.0))[0]
    else:
        scan_host = S.make_scene(cfg, seed=0, extent=(8.0, 6.0, 3.0), n_points=args.points)[0]
    scan = scan_host.cuda()
    learner = ProtoLearner(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
    learner.fit(S.make_episode(cfg, seed=0, noise_ratio=0.2)[0][:2])
    predict = lambda: learner.predict_scene(scan, block_size=1.0)
    out = {"points": args.points, "calls": args.calls, "voxel": args.voxel, "scan": args.scan,
           "predict_scene": timed_calls(predict, min(args.calls, 3)), "runs": []}
    res = predict()
    configs = [(6, None, None, None), (26, None, None, None), (6, args.colour_tol, None, None), (26, args.colour_tol, None, None),
               (6, 0.0, None, None), (26, 0.0, None, None)]
    if args.normal_tol is not None:
        configs += [(conn, tol, args.normal_tol, None) for conn, tol, _, _ in configs[:4]]
    configs += [(conn, None, args.normal_tol, rings) for conn in (6, 26) for rings in [0] + args.absorb if args.absorb]
    for n, (conn, tol, ntol, rings) in enumerate(configs):
        if ntol is None:  # (the call of a tree that has no normal_tol, too)
            grow = lambda: G.build_segments(scan, voxel=args.voxel, colour_tol=tol, connectivity=conn)
        elif rings is None:  # (and of one that has no absorb)
            grow = lambda: G.grow_segments(scan, voxel=args.voxel, colour_tol=tol, connectivity=conn, normal_tol=ntol)
        else:
            grow = lambda: G.absorb_segments(scan, voxel=args.voxel, colour_tol=tol, connectivity=conn, normal_tol=ntol,
                                             min_points=args.min_points, absorb=rings)
        rec = {"connectivity": conn, "colour_tol": tol, "normal_tol": ntol, "build_segments": timed_calls(grow, args.calls)}
        rec["span_ms"] = spans(grow, args.calls)
        sg = grow()
        rec.update(n_voxels=sg.n_voxels, n_components=sg.n_components, n_segments=sg.n_segments, grid=list(sg.grid),
                   largest_segment_points=sorted(sg.segment_points.tolist(), reverse=True)[:6])
        if ntol is not None:
            rec["voxels_without_normal"] = int(torch.isnan(sg.voxel_normals[:, 0]).sum())
        if rings is not None:
            rec.update(min_points=args.min_points, absorb=rings, n_absorbed_voxels=sg.n_absorbed_voxels,
                       n_absorbed_points=sg.n_absorbed_points, n_dropped_points=sg.n_dropped_points,
                       share_unsegmented=round(float((sg.segments < 0).float().mean()), 6))
        rec["pool_segments"] = timed_calls(lambda: SS.pool_segments(res, sg.segments), args.calls)
        if (args.baseline == "all" and (n < 4 or ntol is not None)) or (args.baseline == "one" and n == 0):
            t0 = time.perf_counter()
            if ntol is None:
                import scene_grow_ref
                want = scene_grow_ref.grow(scan_host.numpy(), args.voxel, tol, conn)
            elif rings is not None:
                import scene_grow_absorb_ref
                want = scene_grow_absorb_ref.grow(scan_host.numpy(), args.voxel, tol, conn, args.min_points, ntol, rings)
            else:
                import scene_grow_normals_ref
                want = scene_grow_normals_ref.grow(scan_host.numpy(), args.voxel, tol, conn, normal_tol=ntol)
            rec["numpy_restatement_host_s"] = round(time.perf_counter() - t0, 2)
            rec["equals_restatement"] = bool(np.array_equal(sg.segments.cpu().numpy(), want["segments"])
                                             and np.array_equal(sg.voxel_index.cpu().numpy(), want["voxel_index"])
                                             and sg.n_components == want["n_components"])
        out["runs"].append(rec)
        print("connectivity %d, colour_tol %s, normal_tol %s, absorb %s: done" % (conn, tol, ntol, rings), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
