"""Where the time of learner.predict_scene goes: a seeded room of about 1 M points (8 m x 6 m), block_size 1.0, workload-S
models (pc_npts 2048), MPTILearner_V3 (fitted with eval=True) and ProtoLearner.

    python tools/scene_label_cost.py [--points 1000000] [--extent 8 6 3] [--block-size 1.0] [--stride S] [--groups 32]
                                     [--calls 3] [--max-chunks-per-block C] [--transfer nearest|idw] [--sweep]

The whole call is timed with one HIP event pair per call (it contains the plan's two host reads and, for MPTI, one
convergence read per launch).  The spans -- plan, chunk preparation, predict launches, vote -- are bracketed by event pairs
THIS TOOL puts around scene.ScenePlan's constructor / prepare / vote and around the learner's launch hook while it runs;
the product path records nothing.  Per span the tool also reports the bytes the algorithm has to move (what each kernel
must read and write once, gathers counted per element) and that over the span's time.  For the predict span only the
clouds in and the logits out are counted, not the network's own traffic, so its figure is no bandwidth.  With
transfer="nearest" or "idw" a fifth span brackets ScenePlan.transfer (its kernels; the read of its count comes after).

--sweep measures, in one run, max_chunks_per_block = None, 4, 2 and 1, each without the transfer, with "nearest" and with
"idw", and reports for every capped run the share of scan points whose label equals the uncapped run's label with the
same transfer setting (`agree`), and the share that has a label at all (`labelled`).  Prints one JSON line."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import scene, synthetic as S  # noqa: E402


class Spans:
    """Event pairs around the four spans of one predict_scene call."""

    def __init__(self, learner):
        self.learner, self.plan = learner, None
        self.events = {k: [] for k in ("plan", "prepare", "predict", "vote", "transfer")}
        self._orig = (scene.ScenePlan.__init__, scene.ScenePlan.prepare, scene.ScenePlan.vote, learner._scene_launch,
                      scene.ScenePlan.transfer)

    def _wrap(self, name, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.events[name].append((e0, e1))
            return out
        return timed

    def __enter__(self):
        init, prepare, vote, launch, transfer = self._orig
        spans = self

        def plan_init(plan, *a, **k):
            spans.plan = plan
            return spans._wrap("plan", init)(plan, *a, **k)
        scene.ScenePlan.__init__ = plan_init
        scene.ScenePlan.prepare = self._wrap("prepare", prepare)
        scene.ScenePlan.vote = self._wrap("vote", vote)
        scene.ScenePlan.transfer = self._wrap("transfer", transfer)
        self.learner._scene_launch = self._wrap("predict", launch)
        return self

    def __exit__(self, *exc):
        scene.ScenePlan.__init__, scene.ScenePlan.prepare, scene.ScenePlan.vote = self._orig[:3]
        scene.ScenePlan.transfer = self._orig[4]
        del self.learner._scene_launch  # the instance attribute: the class's method shows again

    def ms(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.events.items()}


def needed_bytes(plan, ld, C, K, transfer=None):
    """Bytes each span has to move once (4-byte words)."""
    M, N, n = plan.M, plan.N, plan.n_run
    # "idw": three int64 neighbours and three weights per point from the flags pass; per receiver three vote counts and three
    # score rows in instead of one row, and its neighbours and weights out again
    idw = 4 * M * 9 + 4 * (M - plan.n_voted) * (3 + 2 * K + 9) if transfer == "idw" else 0
    passes = 1 if plan.n_cells < 256 else (2 if plan.n_cells < 65536 else 3)
    return {
        # bounds and keys read the scan rows; keys write (key, index); a pass reads keys for the counts, then reads and
        # writes the pairs; the cell pass reads the sorted pairs and writes a position per point
        "plan": 4 * M * (2 * ld + 2 + passes * 5 + 3),
        # per slot: its position in the sorted order, its scan row (the second pass hits the cache), C channels out
        "prepare": 4 * n * N * (1 + ld + C),
        "predict": 4 * n * N * (C + K),
        # logits once; per point its sorted position and key in, K scores, an int64 label and a count out
        "vote": 4 * (n * K * N + M * (2 + K + 2 + 1)),
        # flags, scan and compaction: order and votes in, offsets in and out, a 4-word row or an index out, an int64 source;
        # then per receiver its row in and K scores, a label and a source out.  The candidate rows a workgroup stages are
        # re-read by every tile of a cell and are not counted: the span is arithmetic, not traffic
        "transfer": 4 * M * (2 + 3 + 4 + 2) + 4 * (M - plan.n_voted) * (1 + 3 + 2 * K + 4) + idw,
    }


def measure(learner, scan, kw, calls, cfg):
    """One configuration: a warm-up call, `calls` timed calls, one call with the spans -> (record, labels)."""
    res = learner.predict_scene(scan, **kw)  # warm-up: allocations, the label propagation's launch budget
    torch.cuda.synchronize()
    whole = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = learner.predict_scene(scan, **kw)
        b.record()
        torch.cuda.synchronize()
        whole.append(a.elapsed_time(b))
    with Spans(learner) as sp:
        res = learner.predict_scene(scan, **kw)
        span_ms = sp.ms()
    need = needed_bytes(sp.plan, scan.shape[1], cfg["pc_in_dim"], cfg["n_way"] + 1, kw["transfer"])
    total = sum(span_ms.values())
    return {
        "max_chunks_per_block": kw["max_chunks_per_block"], "transfer": kw["transfer"],
        "n_blocks": res.n_blocks, "n_chunks": res.n_chunks, "n_chunks_skipped": res.n_chunks_skipped,
        "n_transferred": res.n_transferred, "n_unlabelled": res.n_unlabelled, "redone": res.redone,
        "launches": len(sp.events["predict"]),
        "call_ms": {"mean": sum(whole) / len(whole), "best": min(whole)},
        "span_ms": {k: round(v, 4) for k, v in span_ms.items()},
        "span_needed_bytes": need,
        "span_needed_GB_per_s": {k: round(need[k] / (span_ms[k] * 1e6), 2) if span_ms[k] > 0 else None for k in need},
        "share_not_predict": round(1.0 - span_ms["predict"] / total, 4) if total > 0 else None,
    }, res.labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--extent", type=float, nargs=3, default=[8.0, 6.0, 3.0])
    ap.add_argument("--block-size", type=float, default=1.0)
    ap.add_argument("--stride", type=float, default=None)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--max-chunks-per-block", type=int, default=None)
    ap.add_argument("--transfer", choices=["nearest", "idw"], default=None)
    ap.add_argument("--sweep", action="store_true", help="max_chunks_per_block None, 4, 2, 1, each without the transfer, with nearest and with idw")
    args = ap.parse_args()
    cfg = S.workload_cfg("S")
    scan = S.make_scene(cfg, seed=0, extent=tuple(args.extent), n_points=args.points)[0].cuda()
    support = S.make_episode(cfg, seed=0, noise_ratio=0.2)[0][:2]
    kw = dict(block_size=args.block_size, stride=args.stride, groups_per_launch=args.groups)
    out = {"points": args.points, "extent": args.extent, "block_size": args.block_size, "stride": args.stride or args.block_size,
           "pc_npts": cfg["pc_npts"], "groups_per_launch": args.groups, "calls": args.calls}
    configs = [(args.max_chunks_per_block, args.transfer)]
    if args.sweep:
        configs = [(c, t) for c in (None, 4, 2, 1) for t in (None, "nearest", "idw")]
    for name in ("mpti", "protonet"):
        if name == "mpti":
            from r3dfsseg_amd.mpti_learner import MPTILearner_V3 as L
            fit_kw = {"eval": True}
        else:
            from r3dfsseg_amd.proto_learner import ProtoLearner as L
            fit_kw = {}
        learner = L(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
        learner.fit(support, **fit_kw)
        runs, uncapped = [], {}
        for cap, transfer in configs:
            rec, labels = measure(learner, scan, dict(kw, max_chunks_per_block=cap, transfer=transfer), args.calls, cfg)
            if cap is None:
                uncapped[transfer] = labels
            elif transfer in uncapped:
                rec["agree"] = round(float((labels == uncapped[transfer]).float().mean()), 6)
            rec["labelled"] = round(float((labels >= 0).float().mean()), 6)
            runs.append(rec)
        out[name] = runs if args.sweep else runs[0]
        del learner, uncapped
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
