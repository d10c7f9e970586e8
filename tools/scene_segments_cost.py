"""What scene_segments.pool_segments costs on a scan of about 1 M points, beside the torch formulation of the same step and
beside the predict_scene call whose result it pools.

    python tools/scene_segments_cost.py [--points 1000000] [--calls 5] [--cols 3 63] [--mixes small mixed giant]

res: ProtoLearner.predict_scene (workload S, 2 ways, so 3 score columns) on a seeded room of 8 m x 6 m, timed with one event
pair per call; for another column count the votes and labels of that result with seeded random scores of that many columns
(pool_segments reads nothing else of res).  segments, seeded, a point's id independent of its place in the scan (the
members of a segment are scattered over the scan: the gather's worst case), 5 % of the points in no segment:
  small   segments of about 50 points;
  mixed   sizes drawn log-uniformly from 10 to 20 000;
  giant   one segment holding half the scan, the rest as `small`.

Per configuration, after a warm-up call: `calls` calls each timed with one HIP event pair (the call's three host reads lie
inside it) and with the host clock; then one call with event pairs THIS TOOL puts around the ops wrappers -- sort (ids +
group), pool, spread -- and the host clock around the three record reads (a read waits for what is queued in front of it,
so it is at least that device time).  The torch baseline on the same inputs and device: torch.sort(stable=True) of the ids,
unique_consecutive, index_add_ of the contributors' rows (floating-point atomics: its summation order is not fixed), a
division, arg-max and an index back per point.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import ops, scene, scene_segments as SS, synthetic as S  # noqa: E402


def make_segments(mix, M, seed):
    rs = np.random.RandomState(seed)
    if mix == "small":
        sizes = np.full(M // 50 + 1, 50)
    elif mix == "mixed":
        sizes = np.exp(rs.uniform(np.log(10), np.log(20000), M // 10 + 1)).astype(np.int64)
    else:
        sizes = np.concatenate([[M // 2], np.full(M // 100 + 1, 50)])
    ids = np.repeat(np.arange(len(sizes)), sizes)[:M]
    assert len(ids) == M, (mix, len(ids))
    ids = ids[rs.permutation(M)]
    ids[rs.rand(M) < 0.05] = -1
    return torch.from_numpy(ids.astype(np.int64)).cuda()


def torch_pool(scores, votes, labels, seg, min_members=1):
    """The same step in torch: grouped by a stable sort, summed by index_add_ (atomics)."""
    M, C = scores.shape
    order = torch.sort(seg, stable=True).indices
    sorted_ids = seg[order]
    uniq, inv_sorted = torch.unique_consecutive(sorted_ids, return_inverse=True)
    first = 1 if uniq.numel() and uniq[0] < 0 else 0  # row 0 collects the points of no segment (ids are all -1 here)
    row = torch.empty(M, dtype=torch.int64, device=seg.device)
    row[order] = inv_sorted
    contrib = (seg >= 0) & (votes > 0)
    rows = scores[contrib] / votes[contrib, None].float()
    sums = torch.zeros(uniq.numel(), C, device=seg.device).index_add_(0, row[contrib], rows)
    members = torch.zeros(uniq.numel(), device=seg.device).index_add_(0, row[contrib], torch.ones_like(rows[:, 0]))
    mean = sums / members.clamp(min=1)[:, None]
    seg_labels = torch.where(members > 0, mean.argmax(1), torch.full_like(members, -1, dtype=torch.int64))
    pooled = (seg >= 0) & (members[row] >= min_members)
    out_scores = torch.where(pooled[:, None], mean[row], scores)
    out_labels = torch.where(pooled, seg_labels[row], labels)
    return out_scores, out_labels, uniq[first:], mean[first:]


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
    return {"event_ms": {"mean": round(sum(dev) / calls, 4), "best": round(min(dev), 4)},
            "host_ms": {"mean": round(sum(host) / calls, 4), "best": round(min(host), 4)}}


def spans(res, seg):
    """One call with event pairs around the ops wrappers and the host clock around the record reads."""
    events, reads = {"sort": [], "pool": [], "spread": []}, []
    orig = {n: getattr(ops, n) for n in ("scene_seg_ids", "scene_seg_group", "scene_seg_pool", "scene_seg_spread")}
    read = SS.read_record

    def wrap(span, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            events[span].append((e0, e1))
            return out
        return timed

    def timed_read(ws):
        t0 = time.perf_counter()
        out = read(ws)
        reads.append((time.perf_counter() - t0) * 1e3)
        return out
    try:
        ops.scene_seg_ids, ops.scene_seg_group = wrap("sort", orig["scene_seg_ids"]), wrap("sort", orig["scene_seg_group"])
        ops.scene_seg_pool, ops.scene_seg_spread = wrap("pool", orig["scene_seg_pool"]), wrap("spread", orig["scene_seg_spread"])
        SS.read_record = timed_read
        out = SS.pool_segments(res, seg)
        torch.cuda.synchronize()
    finally:
        for n, fn in orig.items():
            setattr(ops, n, fn)
        SS.read_record = read
    ms = {k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in events.items()}
    ms["host_reads"] = [round(r, 4) for r in reads]
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cols", type=int, nargs="+", default=[3, 63])
    ap.add_argument("--mixes", nargs="+", default=["small", "mixed", "giant"], choices=["small", "mixed", "giant"])
    args = ap.parse_args()
    from r3dfsseg_amd.proto_learner import ProtoLearner
    cfg = S.workload_cfg("S")
    scan = S.make_scene(cfg, seed=0, extent=(8.0, 6.0, 3.0), n_points=args.points)[0].cuda()
    learner = ProtoLearner(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
    learner.fit(S.make_episode(cfg, seed=0, noise_ratio=0.2)[0][:2])
    predict = lambda: learner.predict_scene(scan, block_size=1.0)
    out = {"points": args.points, "calls": args.calls, "predict_scene": timed_calls(predict, min(args.calls, 3))}
    real = predict()
    M = real.scores.shape[0]
    out["voted_share"] = round(float((real.votes > 0).float().mean()), 4)
    out["runs"] = []
    for cols in args.cols:
        if cols == real.scores.shape[1]:
            res = real
        else:
            g = torch.Generator(device="cuda").manual_seed(cols)
            scores = torch.randn(M, cols, device="cuda", generator=g) * real.votes.clamp(min=1)[:, None].float()
            res = scene.SceneResult(real.labels, scores, real.votes, real.n_blocks, real.n_chunks, real.n_unlabelled, 0)
        for n, mix in enumerate(args.mixes):
            seg = make_segments(mix, M, seed=n)
            rec = {"cols": cols, "mix": mix}
            rec["pool_segments"] = timed_calls(lambda: SS.pool_segments(res, seg), args.calls)
            rec["span_ms"], got = spans(res, seg)
            rec["torch"] = timed_calls(lambda: torch_pool(res.scores, res.votes, res.labels, seg), args.calls)
            rec["n_segments"], rec["n_pooled"] = got.n_segments, got.n_pooled
            rec["largest_segment_members"] = int(got.segment_members.max())
            # the two formulations agree up to the summation order: said here so that the baseline is known to do the same work
            t_scores, t_labels, t_ids, t_mean = torch_pool(res.scores, res.votes, res.labels, seg)
            assert torch.equal(t_ids, got.segment_ids)
            rec["max_abs_diff_to_torch"] = float((t_mean - got.segment_scores).abs().max())
            rec["labels_equal_share"] = round(float((t_labels == got.labels).float().mean()), 6)
            p, t = rec["pool_segments"]["event_ms"]["mean"], rec["torch"]["event_ms"]["mean"]
            rec["ratio_to_torch"] = round(p / t, 4)
            rec["ratio_to_predict_scene"] = round(p / out["predict_scene"]["event_ms"]["mean"], 6)
            out["runs"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
