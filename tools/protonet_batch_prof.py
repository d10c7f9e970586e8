"""ProtoNet episodes per second: ProtoLearner.train / test one episode per call against train_batch / test_batch of E
episodes per call, workload S shape (2-way 5-shot, 2048 points, attention on), synthetic weights and episodes.

    python tools/protonet_batch_prof.py                      # single calls and E = 8, 32; one JSON line per leg
    python tools/protonet_batch_prof.py --legs single        # runs on a commit without train_batch / test_batch as well
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/protonet_batch_prof.py --legs trace --E 32

Event-timed on the current stream after a warm-up; every leg starts from the same weights and uses the same episodes
(episode i of a leg is episode i mod 32 of one fixed list).  `--legs trace`: a few test_batch calls and E test calls, nothing
timed -- for a kernel trace that shows the batched head's kernels next to E launches of the single head's."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import synthetic as S  # noqa: E402
from r3dfsseg_amd.proto_learner import ProtoLearner  # noqa: E402

N_EPISODES = 32


def _learner(cfg):
    return ProtoLearner(SimpleNamespace(**cfg), mode="train")


def _timed(fn, n, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(warmup + i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="single,batch", help="comma list of single, batch, trace")
    ap.add_argument("--E", default="8,32", help="episodes per batched call")
    ap.add_argument("--episodes", type=int, default=128, help="episodes per timed leg")
    ap.add_argument("--warmup", type=int, default=32, help="episodes before the timed ones")
    args = ap.parse_args()
    legs = args.legs.split(",")
    Es = [int(e) for e in args.E.split(",")]
    cfg = S.workload_cfg("S", pretrain_checkpoint_path="synthetic", model_checkpoint_path=None, lr=1e-3, step_size=5000, gamma=0.5)
    eps = []
    for i in range(N_EPISODES):
        data, _ = S.make_episode(cfg, seed=100 + i, noise_ratio=0.4, train=True)
        eps.append([t.cuda() for t in data])
    tests = [ep[:4] + [None, None, ep[6]] for ep in eps]
    shape = dict(n_way=cfg["n_way"], k_shot=cfg["k_shot"], n_points=cfg["pc_npts"], n_query=int(eps[0][2].shape[0]))

    def report(leg, E, n, secs):
        print(json.dumps(dict(leg=leg, E=E, episodes=n, seconds=round(secs, 4), episodes_per_s=round(n / secs, 1), **shape)), flush=True)

    if "single" in legs:
        L = _learner(cfg)
        secs = _timed(lambda i: L.train(eps[i % N_EPISODES], None), args.episodes, args.warmup)
        report("train", 1, args.episodes, secs)
        L = _learner(cfg)
        secs = _timed(lambda i: L.test(tests[i % N_EPISODES], None), args.episodes, args.warmup)
        report("test", 1, args.episodes, secs)
    if "batch" in legs:
        for E in Es:
            calls, warm = max(1, args.episodes // E), max(2, args.warmup // E)
            L = _learner(cfg)
            secs = _timed(lambda i: L.train_batch([eps[(i * E + j) % N_EPISODES] for j in range(E)], None), calls, warm)
            report("train_batch", E, calls * E, secs)
            L = _learner(cfg)
            secs = _timed(lambda i: L.test_batch([eps[(i * E + j) % N_EPISODES] for j in range(E)]), calls, warm)
            report("test_batch", E, calls * E, secs)
    if "trace" in legs:
        E = Es[-1]
        L = _learner(cfg)
        for _ in range(3):
            L.test_batch(eps[:E])
        for e in range(E):
            L.test(tests[e], None)
        torch.cuda.synchronize()
        print(json.dumps(dict(leg="trace", test_batch_calls=3, E=E, test_calls=E)), flush=True)


if __name__ == "__main__":
    main()
