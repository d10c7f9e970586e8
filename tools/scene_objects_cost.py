"""What scene_objects.extract_objects costs on a room of about 1 M points, span by span, beside build_segments on the same
scan with the same voxel and connectivity -- the call that does the same sort and union without the class in the key and
without the object table.

    python tools/scene_objects_cost.py [--points 1000000] [--calls 9] [--voxel 0.05] [--min-points 1] [--check]

The scan is synthetic.make_room(seed=0, n_points, extent=(8, 6, 3)): a floor (class 0), four walls (class 1) and three boxes
(class 2), labelled from its surface column.  Per connectivity (6, 26), by the method of tools/scene_grow_cost.py: after a
warm-up call, `calls` calls each between one HIP event pair (the call's four host reads lie inside it) and the host clock,
reported as median, minimum and maximum; then `calls` more with event pairs THIS TOOL puts around the ops wrappers -- bounds
(with the labels), sort (keys, radix sort, heads, scan, unit table), union, flatten (roots, counts, kept flags, scan), stats
(fill, the per-unit reduction with its atomics, finish), ids -- and the host clock around the record reads.  build_segments
is timed the same way.  Also per connectivity: the objects, their classes and sizes, and the atomics the stats kernel sends
(10 per wave of 64 unit rows and distinct kept object in it, counted on the host from the result).  --check: every field
against the numpy restatement tests/scene_objects_ref.py (a minute or so of one CPU core).  Prints one JSON line."""
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

from r3dfsseg_amd import ops, scene_grow as G, scene_objects as SO, synthetic as S  # noqa: E402

OBJ_SPANS = {"scene_obj_bounds": "bounds", "scene_obj_sort": "sort", "scene_obj_union": "union",
             "scene_obj_components": "flatten", "scene_obj_stats": "stats", "scene_obj_ids": "ids"}
GROW_SPANS = {"scene_grow_bounds": "bounds", "scene_grow_sort": "sort", "scene_grow_voxels": "voxels", "scene_grow_union": "union",
              "scene_grow_components": "flatten", "scene_grow_ids": "ids"}


def spans(fn, calls, names, module):
    """`calls` calls with event pairs around the ops wrappers in `names` and the host clock around module.read_record ->
    medians per span."""
    orig = {n: getattr(ops, n) for n in names}
    read = module.read_record
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
                setattr(ops, n, wrap(names[n], f, events))
            module.read_record = timed_read
            fn()
            torch.cuda.synchronize()
        finally:
            for n, f in orig.items():
                setattr(ops, n, f)
            module.read_record = read
        runs.append({span: e0.elapsed_time(e1) for span, e0, e1 in events})
        reads.append(this_reads)
    out = {span: stats([r[span] for r in runs]) for span in dict.fromkeys(names.values()) if span in runs[0]}
    out["host_reads_median"] = [round(float(np.median([r[i] for r in reads])), 4) for i in range(len(reads[0]))]
    return out


def stats_atomics(objs):
    """10 atomics (6 min / max, 3 64-bit adds, 1 add) per wave of 64 unit rows and distinct kept object in it."""
    unit_object = torch.full((objs.n_units,), -1, dtype=torch.int64, device=objs.objects.device)
    on = objs.unit_index >= 0
    unit_object[objs.unit_index[on].long()] = objs.objects[on].long()
    wave = torch.arange(objs.n_units, device=unit_object.device) // 64
    kept = unit_object >= 0
    pairs = torch.unique(wave[kept] * (objs.n_objects + 1) + unit_object[kept]).numel()
    return {"waves": int((objs.n_units + 63) // 64), "wave_object_pairs": pairs, "atomics": 10 * pairs,
            "atomics_one_set_per_unit": 10 * int(kept.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--min-points", type=int, default=1)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import scene_objects_cases as OC
    scan_host, surface = S.make_room(seed=0, n_points=args.points, extent=(8.0, 6.0, 3.0))
    labels_host = torch.from_numpy(OC.labels_of_surface(surface.numpy()))
    scan, labels = scan_host.cuda(), labels_host.cuda()
    out = {"points": args.points, "calls": args.calls, "voxel": args.voxel, "min_points": args.min_points, "runs": []}
    for conn in (6, 26):
        extract = lambda: SO.extract_objects(scan, labels, voxel=args.voxel, connectivity=conn, min_points=args.min_points)
        grow = lambda: G.build_segments(scan, voxel=args.voxel, connectivity=conn, min_points=args.min_points)
        rec = {"connectivity": conn, "extract_objects": timed_calls(extract, args.calls),
               "extract_objects_span_ms": spans(extract, args.calls, OBJ_SPANS, SO),
               "build_segments": timed_calls(grow, args.calls), "build_segments_span_ms": spans(grow, args.calls, GROW_SPANS, G)}
        objs, sg = extract(), grow()
        order = torch.argsort(objs.object_points, descending=True)[:12]
        rec.update(grid=list(objs.grid), n_labels=objs.n_labels, n_units=objs.n_units, n_components=objs.n_components,
                   n_objects=objs.n_objects, n_dropped_points=objs.n_dropped_points, n_voxels=sg.n_voxels,
                   n_segments=sg.n_segments, objects_per_class=torch.bincount(objs.object_labels, minlength=3).tolist(),
                   largest_objects=[{"class": int(objs.object_labels[i]), "points": int(objs.object_points[i]),
                                     "units": int(objs.object_units[i])} for i in order.tolist()],
                   stats_kernel=stats_atomics(objs))
        if args.check:
            import scene_objects_ref as OR
            t0 = time.perf_counter()
            want = OR.extract(scan_host.numpy(), labels_host.numpy(), args.voxel, conn, args.min_points)
            rec["numpy_restatement_host_s"] = round(time.perf_counter() - t0, 2)
            same = all(np.array_equal(getattr(objs, k).cpu().numpy(), want[k]) for k in
                       ("objects", "unit_index", "object_labels", "object_points", "object_units"))
            same = same and all(np.array_equal(getattr(objs, k).cpu().numpy().view(np.uint32), want[k].view(np.uint32))
                                for k in ("object_lo", "object_hi", "object_centroid"))
            same = same and all(getattr(objs, k) == want[k] for k in
                                ("n_objects", "n_units", "n_components", "n_dropped_points", "n_unlabelled", "n_invalid",
                                 "n_labels", "grid"))
            rec["equals_restatement"] = bool(same)
        out["runs"].append(rec)
        print("connectivity %d: done" % conn, file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
