"""What fitting the support set once saves an evaluation call: HIP-event time of learner.test_batch on E episodes of one
workload that SHARE one support set, against learner.fit once + learner.predict on the same E query groups, for
MPTILearner_V3 (eval=True) and ProtoLearner; and per entry point (ops.KernelTimer) where the time of each goes.

    python tools/fitted_predict_cost.py [--episodes 32] [--workload S] [--iters 10] [--test-batch-only]

Every timed call ends with the learner's host read, so a round of `iters` calls between one event pair is end-to-end time.
Prints one JSON line.  --test-batch-only: the test_batch leg alone (runs on a tree without fitted.py: the parent's number)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import ops, synthetic as S  # noqa: E402

ENTRY_POINTS = ["knn_topk", "knn_topk_l2", "pointwise_conv", "edgeconv", "attention", "head_prototypes", "label_propagate",
                "head_attach_queries", "protonet_prototypes", "protonet_similarity"]


def timed(fn, iters, warmup=3):
    """Per-call ms: mean over `iters` back-to-back calls between one event pair, mean and best of 5 such rounds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    rounds = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        rounds.append(a.elapsed_time(b) / iters)
    return {"mean_ms": sum(rounds) / len(rounds), "best_ms": min(rounds)}


def per_entry_point(fn):
    """Total ms per timed entry point of ONE call of fn (an event pair around every library call)."""
    t = ops.KernelTimer(ENTRY_POINTS)
    ops.set_timer(t)
    try:
        fn()
        s = t.summary()
    finally:
        ops.set_timer(None)
        t.close()
    return {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 4)} for k, v in s.items() if v["launches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=32)
    ap.add_argument("--workload", default="S")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--test-batch-only", action="store_true")
    args = ap.parse_args()
    cfg = S.workload_cfg(args.workload)
    E = args.episodes
    support = [t.cuda() for t in S.make_episode(cfg, seed=0, noise_ratio=0.2)[0][:2]]
    groups = [[t.cuda() for t in S.make_episode(cfg, seed=100 + e)[0][2:4]] for e in range(E)]
    episodes = [support + g for g in groups]
    QX, QY = torch.stack([g[0] for g in groups]), torch.stack([g[1] for g in groups])
    out = {"workload": args.workload, "episodes": E, "support_clouds": cfg["n_way"] * cfg["k_shot"],
           "query_clouds_per_group": int(QX.shape[1]), "points": cfg["pc_npts"]}
    for name in ("mpti", "protonet"):
        if name == "mpti":
            from r3dfsseg_amd.mpti_learner import MPTILearner_V3 as L
            kw = {"eval": True}
        else:
            from r3dfsseg_amd.proto_learner import ProtoLearner as L
            kw = {}
        learner = L(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
        from r3dfsseg_amd.batch import EpisodeBatch
        batch = EpisodeBatch.from_episodes(episodes)
        res = {"test_batch": timed(lambda: learner.test_batch(batch, **kw), args.iters)}
        res["test_batch_entry_points"] = per_entry_point(lambda: learner.test_batch(batch, **kw))
        if not args.test_batch_only:
            res["fit"] = timed(lambda: learner.fit(support, **kw), args.iters)
            learner.fit(support, **kw)
            res["predict"] = timed(lambda: learner.predict(QX, QY), args.iters)
            res["fit_entry_points"] = per_entry_point(lambda: learner.fit(support, **kw))
            res["predict_entry_points"] = per_entry_point(lambda: learner.predict(QX, QY))
            a, b = learner.test_batch(batch, **kw), learner.predict(QX, QY)
            res["predict_equals_test_batch"] = all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and x[2] == y[2]
                                                   for x, y in zip(a, b))
        out[name] = res
        del learner
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
