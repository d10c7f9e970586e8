"""What the device augmentation costs per training step: HIP-event time of EpisodeBatch.augmented on the benchmark's batch
(E = 32 episodes of workload S, resident on the device), and of the r3d_augment_clouds launch alone, for both input layouts.

    python tools/augment_cost.py [--episodes 32] [--workload S] [--iters 50]

Prints one JSON line; set it beside the training-step time `bench.py --gpus 1` reports."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import synthetic as S  # noqa: E402
from r3dfsseg_amd.augment import augment_clouds  # noqa: E402
from r3dfsseg_amd.batch import EpisodeBatch  # noqa: E402

CFG = {"scale": 1.2, "rot": 1, "mirror_prob": 1.0, "jitter": 1}


def timed(fn, iters, warmup=5):
    """Per-call ms (mean over `iters` back-to-back calls between one event pair, and the best of 5 such rounds)."""
    for _ in range(warmup):
        fn(0)
    torch.cuda.synchronize()
    rounds = []
    for r in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(iters):
            fn(r * iters + i)
        b.record()
        torch.cuda.synchronize()
        rounds.append(a.elapsed_time(b) / iters)
    return {"mean_ms": sum(rounds) / len(rounds), "best_ms": min(rounds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=32)
    ap.add_argument("--workload", default="S")
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    cfg = S.workload_cfg(args.workload)
    eps = []
    for e in range(args.episodes):
        data, _ = S.make_episode(cfg, seed=e, noise_ratio=0.2, train=True)
        eps.append([t.cuda() for t in data])
    out = {"workload": args.workload, "episodes": args.episodes}
    for layout in ("channel_major", "point_major"):
        if layout == "point_major":
            for ep in eps:
                for i in (0, 2):
                    ep[i] = ep[i].transpose(-1, -2).contiguous().transpose(-1, -2)
        b = EpisodeBatch.from_episodes(eps)
        E, SQ, C, N = b.x_all.shape
        x = b.x_all.reshape(E * SQ, C, N)
        dst = augment_clouds(x, CFG, 1)
        out["clouds"], out["points"], out["channels"] = E * SQ, N, C
        out[layout] = {
            "kernel_only": timed(lambda i: augment_clouds(x, CFG, 1, first_key=i * E * SQ, out=dst), args.iters),
            "EpisodeBatch.augmented": timed(lambda i: b.augmented(CFG, 1, i * E), args.iters),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
