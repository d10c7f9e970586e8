"""What scene_match.match_objects costs on a room of about 1 M points, span by span, beside the same tables built on the host
with numpy.

    python tools/scene_match_cost.py [--points 1000000] [--calls 9] [--voxel 0.05] [--min-points 4] [--check]

The scan is synthetic.make_room(seed=0, n_points, extent=(8, 6, 3)), labelled from its surface column (floor 0, walls 1, boxes
2).  truth: extract_objects on those labels; pred: extract_objects on the labels with a band of heights flipped to class 1
(tests/scene_match_cases.room_inputs does the same at 20 000 points).  Both columns and both label columns are on the device
before the clock starts.  By the method of tools/scene_objects_cost.py: after a warm-up call, `calls` calls each between one
HIP event pair (the call's four host reads lie inside it) and the host clock, reported as median, minimum and maximum; then
`calls` more with event pairs THIS TOOL puts around the ops wrappers -- ids, rows (two sorts of (id, scan index), heads, scan,
row tables, mixed rows), pairs (row tables out, two sorts of row keys, heads, scan, pair tables), best -- and the host clock
around the three record reads and the read of the tables.  Once with labels and once without; the room holds a handful of
objects, so a third run matches runs of 64 scan points against runs of 100 (`blocks`: tens of thousands of pairs).  Beside
it, on the room's columns already copied to the host, what a caller would write in numpy: np.unique per column with the
inverse, np.unique over the 64-bit pair keys with counts, the IoU -- the tables of M2 and M4, without classes, best partners
or matches.  --check: every field against the numpy restatement tests/scene_match_ref.py.  Prints one JSON line."""
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

from r3dfsseg_amd import ops, scene_match as SM, scene_objects as SO, synthetic as S  # noqa: E402

MATCH_SPANS = {"scene_match_ids": "ids", "scene_match_rows": "rows", "scene_match_pairs": "pairs", "scene_match_best": "best"}
INT_FIELDS = ("pred_ids", "pred_points", "pred_index", "pred_best", "truth_ids", "truth_points", "truth_index", "truth_best",
              "pair_pred", "pair_truth", "pair_points", "pair_match")
COUNTS = ("n_pred", "n_truth", "n_pairs", "n_pred_unassigned", "n_truth_unassigned", "n_ignored", "n_mixed_pred", "n_mixed_truth")


def host_tables(pred, truth):
    """M2 and M4 as a caller would build them on the host: rows, points, the row of every point, pairs, intersections, IoU."""
    def rows(col):
        on = col >= 0
        ids, inverse, counts = np.unique(col[on], return_inverse=True, return_counts=True)
        index = np.full(len(col), -1, np.int32)
        index[on] = inverse
        return ids, counts.astype(np.int32), index
    pred_ids, pred_points, pred_index = rows(pred)
    truth_ids, truth_points, truth_index = rows(truth)
    both = (pred_index >= 0) & (truth_index >= 0)
    keys, inter = np.unique(pred_index[both].astype(np.int64) * len(truth_ids) + truth_index[both], return_counts=True)
    pair_pred, pair_truth = (keys // len(truth_ids)).astype(np.int32), (keys % len(truth_ids)).astype(np.int32)
    inter = inter.astype(np.int32)
    iou = inter.astype(np.float32) / (pred_points[pair_pred] + truth_points[pair_truth] - inter).astype(np.float32)
    return pred_ids, pred_points, pred_index, truth_ids, truth_points, truth_index, pair_pred, pair_truth, inter, iou


def timed_tables(fn, calls):
    """spans() times the record reads; the read of the tables is timed here, around scene_match.read_tables."""
    read, ms = SM.read_tables, []

    def timed(*a):
        t0 = time.perf_counter()
        out = read(*a)
        ms.append((time.perf_counter() - t0) * 1e3)
        return out
    SM.read_tables = timed
    try:
        out = spans(fn, calls, MATCH_SPANS, SM)
    finally:
        SM.read_tables = read
    out["tables_read_median"] = round(float(np.median(ms)), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--min-points", type=int, default=4)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import scene_objects_cases as OC
    scan_host, surface = S.make_room(seed=0, n_points=args.points, extent=(8.0, 6.0, 3.0))
    labels_host = OC.labels_of_surface(surface.numpy())
    z = scan_host[:, 2].numpy()
    lo = z.min() + 0.3 * (z.max() - z.min())
    flipped_host = np.where((z >= lo) & (z < lo + 0.25), 1, labels_host).astype(np.int64)
    scan, labels, flipped = scan_host.cuda(), torch.from_numpy(labels_host).cuda(), torch.from_numpy(flipped_host).cuda()
    objects = lambda l: SO.extract_objects(scan, l, voxel=args.voxel, connectivity=26, min_points=args.min_points).objects
    truth, pred = objects(labels), objects(flipped)
    out = {"points": args.points, "calls": args.calls, "voxel": args.voxel, "min_points": args.min_points,
           "ws_bytes": 4 * ops.scene_match_workspace(args.points, scan.device).numel(), "runs": []}
    # the room holds a handful of objects; `blocks` gives the pair and best-partner kernels work: runs of 64 scan points as
    # pred, runs of 100 as truth, ids spread so that the sorts take three and two passes
    at = torch.arange(args.points, device=scan.device)
    blocks_pred, blocks_truth = (at // 64 * 7).to(torch.int32), (at // 100 * 3).to(torch.int32)
    for columns, labelled in (("room", True), ("room", False), ("blocks", False)):
        p_col, t_col = (pred, truth) if columns == "room" else (blocks_pred, blocks_truth)
        match = (lambda: SM.match_objects(p_col, t_col, flipped, labels)) if labelled else (lambda: SM.match_objects(p_col, t_col))
        rec = {"columns": columns, "labels": labelled, "match_objects": timed_calls(match, args.calls),
               "match_objects_span_ms": timed_tables(match, args.calls)}
        got = match()
        rec.update({k: getattr(got, k) for k in COUNTS})
        rec["summary_all"] = {str(t): got.summary[t]["all"] for t in got.iou}
        if args.check:
            import scene_match_ref as MR
            t0 = time.perf_counter()
            want = MR.match(p_col.cpu().numpy(), t_col.cpu().numpy(), flipped_host if labelled else None,
                            labels_host if labelled else None)
            rec["numpy_restatement_host_s"] = round(time.perf_counter() - t0, 2)
            same = all(np.array_equal(getattr(got, k).cpu().numpy(), want[k]) for k in INT_FIELDS)
            same = same and np.array_equal(got.pair_iou.cpu().numpy().view(np.uint32), want["pair_iou"].view(np.uint32))
            same = same and all(getattr(got, k) == want[k] for k in COUNTS) and MR.same_summary(got.summary, want["summary"])
            if labelled:
                same = same and all(np.array_equal(getattr(got, k).cpu().numpy(), want[k]) for k in ("pred_classes", "truth_classes"))
            rec["equals_restatement"] = bool(same)
        out["runs"].append(rec)
        print("%s, labels %s: done" % (columns, labelled), file=sys.stderr, flush=True)
    pred_host, truth_host = pred.cpu().numpy(), truth.cpu().numpy()  # copied once, outside the clock
    host_tables(pred_host, truth_host)
    ms = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        tables = host_tables(pred_host, truth_host)
        ms.append((time.perf_counter() - t0) * 1e3)
    got = SM.match_objects(pred, truth)
    out["numpy_host_tables_ms"] = stats(ms)
    out["numpy_host_tables_equal"] = bool(all(np.array_equal(a, getattr(got, k).cpu().numpy()) for a, k in zip(
        tables, ("pred_ids", "pred_points", "pred_index", "truth_ids", "truth_points", "truth_index", "pair_pred", "pair_truth",
                 "pair_points"))) and np.array_equal(tables[9].view(np.uint32), got.pair_iou.cpu().numpy().view(np.uint32)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
