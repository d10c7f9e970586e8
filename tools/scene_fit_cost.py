"""Where the time of learner.fit_scene goes: the seeded room of about 1 M points (8 m x 6 m) of tools/scene_label_cost.py
with the labels synthetic.make_scene returns, classes 1..n_way, block_size 1.0, workload-S models (pc_npts 2048, 2-way
5-shot), MPTILearner_V3 (fitted with eval=True) and ProtoLearner.

    python tools/scene_fit_cost.py [--points 1000000] [--extent 8 6 3] [--block-size 1.0] [--stride S] [--min-fg 100]
                                   [--min-ratio 0.05] [--calls 3] [--labels int64|int32] [--out profiles/r15_scene_fit.md]

The whole call is timed with one HIP event pair per call (it contains the plan's two host reads, the read of the eligible
counts and, for MPTI, the fit's own read).  The spans -- plan, counts + pick, prepare, fit_support -- are bracketed by event
pairs THIS TOOL puts around scene.ScenePlan's constructor, scene_support.count_and_pick, scene_support.prepare_shots and
the model's fit_support while it runs; the product path records nothing.  Prints one JSON line and writes the table to
--out."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import scene, scene_support, synthetic as S  # noqa: E402

SPANS = ("plan", "counts_pick", "prepare", "fit_support")


class Spans:
    """Event pairs around the four spans of one fit_scene call."""

    def __init__(self, learner):
        self.learner, self.plan = learner, None
        self.events = {k: [] for k in SPANS}
        self._orig = (scene.ScenePlan.__init__, scene_support.count_and_pick, scene_support.prepare_shots)

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
        init, count_and_pick, prepare_shots = self._orig
        spans = self

        def plan_init(plan, *a, **k):
            spans.plan = plan
            return spans._wrap("plan", init)(plan, *a, **k)
        scene.ScenePlan.__init__ = plan_init
        scene_support.count_and_pick = self._wrap("counts_pick", count_and_pick)
        scene_support.prepare_shots = self._wrap("prepare", prepare_shots)
        self.learner.model.fit_support = self._wrap("fit_support", self.learner.model.fit_support)
        return self

    def __exit__(self, *exc):
        scene.ScenePlan.__init__, scene_support.count_and_pick, scene_support.prepare_shots = self._orig
        del self.learner.model.fit_support  # the instance attribute: the class's method shows again

    def ms(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.events.items()}


def measure(learner, scan, labels, classes, kw, calls):
    """A warm-up call, `calls` timed calls, one call with the spans -> a record."""
    sup = learner.fit_scene(scan, labels, classes, **kw)
    torch.cuda.synchronize()
    whole = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sup = learner.fit_scene(scan, labels, classes, **kw)
        b.record()
        torch.cuda.synchronize()
        whole.append(a.elapsed_time(b))
    with Spans(learner) as sp:
        sup = learner.fit_scene(scan, labels, classes, **kw)
        span_ms = sp.ms()
    plan = sp.plan
    return {
        "n_blocks": plan.n_blocks, "n_chunks": plan.n_chunks, "n_eligible": sup.n_eligible,
        "shot_block": sup.shot_block.tolist(), "shot_fg": sup.shot_fg.tolist(),
        "mask_points": sup.support_y.sum(-1).tolist(),
        "call_ms": {"mean": sum(whole) / len(whole), "best": min(whole)},
        "span_ms": {k: round(v, 4) for k, v in span_ms.items()},
    }


def table(out):
    rows = ["| learner | whole call, mean / best | plan | counts + pick | prepare | `fit_support` | eligible blocks per way |",
            "|---|---|---|---|---|---|---|"]
    for name in ("mpti", "protonet"):
        r = out[name]
        s = r["span_ms"]
        rows.append("| %s | %.3f / %.3f ms | %.3f | %.3f | %.3f | %.3f | %s |"
                    % (name, r["call_ms"]["mean"], r["call_ms"]["best"], s["plan"], s["counts_pick"], s["prepare"], s["fit_support"],
                       ", ".join(str(n) for n in r["n_eligible"])))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--extent", type=float, nargs=3, default=[8.0, 6.0, 3.0])
    ap.add_argument("--block-size", type=float, default=1.0)
    ap.add_argument("--stride", type=float, default=None)
    ap.add_argument("--min-fg", type=int, default=100)
    ap.add_argument("--min-ratio", type=float, default=0.05)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--labels", choices=["int64", "int32"], default="int64")
    ap.add_argument("--out", default=os.path.join("profiles", "r15_scene_fit.md"))
    args = ap.parse_args()
    cfg = S.workload_cfg("S")
    scan, labels = S.make_scene(cfg, seed=0, extent=tuple(args.extent), n_points=args.points)
    scan, labels = scan.cuda(), labels.to(getattr(torch, args.labels)).cuda()
    classes = list(range(1, cfg["n_way"] + 1))
    kw = dict(block_size=args.block_size, stride=args.stride, min_ratio=args.min_ratio, min_fg=args.min_fg)
    out = {"points": args.points, "extent": args.extent, "block_size": args.block_size, "stride": args.stride or args.block_size,
           "pc_npts": cfg["pc_npts"], "n_way": cfg["n_way"], "k_shot": cfg["k_shot"], "min_ratio": args.min_ratio,
           "min_fg": args.min_fg, "labels": args.labels, "calls": args.calls}
    for name in ("mpti", "protonet"):
        if name == "mpti":
            from r3dfsseg_amd.mpti_learner import MPTILearner_V3 as L
            fit_kw = {"eval": True}
        else:
            from r3dfsseg_amd.proto_learner import ProtoLearner as L
            fit_kw = {}
        learner = L(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
        out[name] = measure(learner, scan, labels, classes, dict(kw, **fit_kw), args.calls)
        del learner
        torch.cuda.empty_cache()
    print(json.dumps(out))
    text = ["# r15 -- `fit_scene`: the support set from an annotated scan, on the device", "",
            "Tool: `python tools/scene_fit_cost.py` (%d points on %g m x %g m, `block_size` %g, stride %g, `pc_npts` %d, %d-way "
            "%d-shot, `min_ratio` %g, `min_fg` %d, %s labels on the device; %d kept blocks, %d chunks).  One warm-up call, the "
            "whole call as one HIP event pair per call (mean / best of %d), then one further call with the tool's event pairs "
            "around the four spans; the span columns are that one call, in ms.  This is one run on one MI355X; nobody has set "
            "a threshold for any figure here, they are recorded as measured."
            % (args.points, args.extent[0], args.extent[1], args.block_size, out["stride"], cfg["pc_npts"], cfg["n_way"], cfg["k_shot"],
               args.min_ratio, args.min_fg, args.labels, out["mpti"]["n_blocks"], out["mpti"]["n_chunks"], args.calls),
            "", table(out), "",
            "Chosen blocks (way by way): %s, with foreground counts %s; mask points per shot %s."
            % (out["mpti"]["shot_block"], out["mpti"]["shot_fg"], out["mpti"]["mask_points"]), "",
            "The JSON line of the run:", "", "```", json.dumps(out), "```", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text))


if __name__ == "__main__":
    main()
