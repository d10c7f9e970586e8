"""What learner.predict_scene_sets costs beside K calls of learner.predict_scene: the seeded room of
tools/scene_label_cost.py (about 1 M points on 8 m x 6 m, block_size 1.0), workload-S models (pc_npts 2048),
MPTILearner_V3 (fitted with eval=True) and ProtoLearner, K = 1, 2, 4 and 6 support sets fitted from K seeded episodes.

    python tools/scene_sets_cost.py [--points 1000000] [--extent 8 6 3] [--block-size 1.0] [--stride S] [--groups 32]
                                    [--calls 3] [--sets 1 2 4 6] [--table]

Both sides are timed with one HIP event pair around the whole work -- one predict_scene_sets call, or the K predict_scene
calls one after the other -- after one warm-up, mean and best of `calls` repeats.  The K-call side is the path that was
there before predict_scene_sets and is its baseline.  One more run of each side is bracketed span by span -- plan, chunk
preparation, predict launches, vote, merge -- by event pairs THIS TOOL puts around scene.ScenePlan's constructor / prepare
/ vote, ops.scene_merge_sets and the learner's launch hooks while it runs; the product path records nothing.  The spans
of the K-call side are sums over its K calls.  Prints one JSON line; --table adds a markdown table of the call times."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import ops, scene, synthetic as S  # noqa: E402


class Spans:
    """Event pairs around the spans of predict_scene / predict_scene_sets calls made inside the `with` block."""
    TARGETS = (("plan", scene.ScenePlan, "__init__"), ("prepare", scene.ScenePlan, "prepare"), ("vote", scene.ScenePlan, "vote"),
               ("merge", ops, "scene_merge_sets"))

    def __init__(self, learner):
        self.learner = learner
        self.events = {k: [] for k in ("plan", "prepare", "predict", "vote", "merge")}

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
        self._orig = [(owner, attr, getattr(owner, attr)) for _, owner, attr in self.TARGETS]
        for (name, owner, attr), (_, _, fn) in zip(self.TARGETS, self._orig):
            setattr(owner, attr, self._wrap(name, fn))
        self.learner._scene_launch = self._wrap("predict", self.learner._scene_launch)
        self.learner._scene_launch_sets = self._wrap("predict", self.learner._scene_launch_sets)
        return self

    def __exit__(self, *exc):
        for owner, attr, fn in self._orig:
            setattr(owner, attr, fn)
        del self.learner._scene_launch, self.learner._scene_launch_sets  # the instance attributes: the class's show again

    def ms(self):
        torch.cuda.synchronize()
        return {k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in self.events.items()}


def timed_calls(fn, calls):
    """One warm-up (allocations, the label propagation's launch budget), then `calls` event pairs -> [ms]."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def measure(learner, scan, fits, kw, calls):
    K = len(fits)
    sets = lambda: learner.predict_scene_sets(scan, fits, **kw)
    singles = lambda: [learner.predict_scene(scan, fitted=f, **kw) for f in fits]
    rec = {"K": K}
    for name, fn in (("sets", sets), ("k_calls", singles)):
        ms = timed_calls(fn, calls)
        with Spans(learner) as sp:
            res = fn()
            spans = sp.ms()
        res = res if isinstance(res, list) else [res]
        rec[name] = {"call_ms": {"mean": round(sum(ms) / len(ms), 4), "best": round(min(ms), 4), "all": [round(v, 4) for v in ms]},
                     "span_ms": spans, "launches": len(sp.events["predict"]), "redone": sum(r.redone for r in res),
                     "n_chunks": res[0].n_chunks}
    rec["sets_over_k_calls"] = round(rec["sets"]["call_ms"]["mean"] / rec["k_calls"]["call_ms"]["mean"], 4)
    rec["sets_over_one_call"] = round(rec["sets"]["call_ms"]["mean"] * K / rec["k_calls"]["call_ms"]["mean"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--extent", type=float, nargs=3, default=[8.0, 6.0, 3.0])
    ap.add_argument("--block-size", type=float, default=1.0)
    ap.add_argument("--stride", type=float, default=None)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 2, 4, 6])
    ap.add_argument("--table", action="store_true", help="print a markdown table of the call times after the JSON line")
    args = ap.parse_args()
    cfg = S.workload_cfg("S")
    scan = S.make_scene(cfg, seed=0, extent=tuple(args.extent), n_points=args.points)[0].cuda()
    kw = dict(block_size=args.block_size, stride=args.stride, groups_per_launch=args.groups)
    out = {"points": args.points, "extent": args.extent, "block_size": args.block_size, "stride": args.stride or args.block_size,
           "pc_npts": cfg["pc_npts"], "n_way": cfg["n_way"], "groups_per_launch": args.groups, "calls": args.calls}
    for name in ("mpti", "protonet"):
        if name == "mpti":
            from r3dfsseg_amd.mpti_learner import MPTILearner_V3 as L
            fit_kw = {"eval": True}
        else:
            from r3dfsseg_amd.proto_learner import ProtoLearner as L
            fit_kw = {}
        learner = L(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
        fits = [learner.fit(S.make_episode(cfg, seed=s, noise_ratio=0.2)[0][:2], **fit_kw) for s in range(max(args.sets))]
        out[name] = [measure(learner, scan, fits[:K], kw, args.calls) for K in args.sets]
        del learner, fits
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.table:
        print("\n| model | K | predict_scene_sets ms (mean / best) | K x predict_scene ms (mean / best) | sets / K calls | sets / one call |")
        print("|---|---|---|---|---|---|")
        for name in ("mpti", "protonet"):
            for r in out[name]:
                a, b = r["sets"]["call_ms"], r["k_calls"]["call_ms"]
                print("| %s | %d | %.2f / %.2f | %.2f / %.2f | %.3f | %.3f |" % (name, r["K"], a["mean"], a["best"], b["mean"],
                                                                               b["best"], r["sets_over_k_calls"],
                                                                               r["sets_over_one_call"]))


if __name__ == "__main__":
    main()
