"""What cutting episodes on the device costs: DeviceEpisodeSampler.batch(E) on workload S (2-way 5-shot, 2048 points, train
mode) against NoiseEpisodeSampler on the same source with its blocks cached in memory.

    python tools/episode_cut_cost.py [--episodes 32] [--iters 20] [--noise train|sym|partial] [--out profiles/NAME.md]

--noise: `train` (the default) is train mode with noise ratios 0 / 0.2 / 0.4; `sym` and `partial` are test mode at noise
ratio 0.4.  The partial leg pools the instance ids and launches r3d_episode_cut_partial; the other two launch
r3d_episode_cut (profiles/r17_episode_partial.md sets the three side by side).

How the time is taken.  batch(): a host clock around calls that end in a device synchronise (the call itself reads the
kernel's record back, so it ends synchronised anyway); after 3 warm-up calls, `iters` calls per round, 5 rounds, mean and
best round.  plan: the host clock around the E plan() calls alone.  launch: HIP events around ops.episode_cut on resident
descriptors (`iters` back-to-back launches between one event pair, 5 rounds) -- the kernel with its record read, without
planning, upload and the two dense copies of EpisodeBatch.  Host sampler: a host clock around episode() calls, one core,
blocks served from a dict.  Prints one JSON line and writes the markdown file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from r3dfsseg_amd import ops  # noqa: E402
from r3dfsseg_amd.block_pool import ATTRIB_SETS, BlockPool, DeviceEpisodeSampler  # noqa: E402
from r3dfsseg_amd.episode_sampler import NoiseEpisodeSampler, SyntheticBlocks  # noqa: E402


class Cached:
    """The source with every block loaded once."""

    def __init__(self, source):
        self.class2scans = source.class2scans
        self.blocks = {n: source.load(n) for c in source.class2scans for n in source.class2scans[c]}

    def load(self, name):
        return self.blocks[str(name)]


def rounds(fn, iters, n_rounds=5, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(n_rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / iters * 1e3)
    return {"mean_ms": sum(out) / len(out), "best_ms": min(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-episodes", type=int, default=40)
    ap.add_argument("--noise", default="train", choices=("train", "sym", "partial"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    E, N = args.episodes, 2048
    classes = list(range(1, 7))
    shape = dict(n_way=2, k_shot=5, n_queries=1, num_point=N, seed=0)
    if args.noise == "train":
        shape.update(mode="train", noise_ratio=[0.0, 0.2, 0.4])
    else:
        shape.update(mode="test", noise_type=args.noise, noise_ratio=0.4)
    partial = args.noise == "partial"
    source = Cached(SyntheticBlocks(classes=classes, scans_per_class=24, points_per_block=3000, seed=0))
    pool = BlockPool.from_source(source, instances=True) if partial else BlockPool.from_source(source)
    res = {"workload": "S", "noise": args.noise, "episodes": E, "clouds": E * 12, "points": N, "blocks": len(pool), "pool_rows": int(pool.points.shape[0])}

    for layout in ("cm", "pm"):
        s = DeviceEpisodeSampler(pool, classes, layout=layout, **shape)
        r = rounds(lambda: s.batch(E), args.iters)
        r["episodes_per_s"] = E / r["mean_ms"] * 1e3
        res["batch_" + layout] = r
    s = DeviceEpisodeSampler(pool, classes, **shape)
    res["plan"] = rounds(lambda: [s.plan() for _ in range(E)], args.iters)

    plans = [s.plan() for _ in range(E)]
    dev = pool.device
    desc = torch.from_numpy(np.concatenate([p.keyed(e) for e, p in enumerate(plans)])).to(dev)
    cls = torch.from_numpy(np.stack([p.sampled_classes for p in plans])).to(dev)
    C, rgb_ch, XYZ_ch = ATTRIB_SETS["xyzrgbXYZ"]
    x = torch.empty(E * 12, C, N, device=dev)
    mask, gt = torch.empty(E * 10, N, device=dev, dtype=torch.int32), torch.empty(E * 10, N, device=dev, dtype=torch.int32)
    qy, gqy = torch.empty(E * 2, N, device=dev, dtype=torch.int64), torch.empty(E * 2, N, device=dev, dtype=torch.int64)
    sm = torch.empty(E * 12, N, device=dev, dtype=torch.int32)
    cut_args = (pool.points, pool.labels, pool.offsets, desc, cls, 10, 2, N, 0, x, rgb_ch, XYZ_ch, mask, gt, qy, gqy, sm)
    if partial:
        info = torch.empty(E * 12, 8, device=dev, dtype=torch.int32)
        launch = lambda: ops.episode_cut_partial(*cut_args, pool.instances, info)
    else:
        launch = lambda: ops.episode_cut(*cut_args)
    for _ in range(3):
        launch()
    ev = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            launch()
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b) / args.iters)
    res["launch"] = {"mean_ms": sum(ev) / len(ev), "best_ms": min(ev)}

    host = NoiseEpisodeSampler(source, classes, **shape)
    for _ in range(3):
        host.episode()
    t = time.perf_counter()
    for _ in range(args.host_episodes):
        host.episode()
    ms = (time.perf_counter() - t) / args.host_episodes * 1e3
    res["host_sampler"] = {"ms_per_episode": ms, "episodes_per_s": 1e3 / ms}
    print(json.dumps(res))
    if args.out:
        b = res["batch_cm"]
        with open(args.out, "w") as f:
            f.write("""# Cutting episodes on the device: what it costs

`python tools/episode_cut_cost.py --episodes %d --iters %d --noise %s` on one MI355X; workload S (2-way 5-shot, 1 query per
way, 2048 points; %s), %d synthetic blocks of 2500 to 3500 points (%d pool rows)
resident on the device; %d clouds per batch.

| what | ms (mean of 5 rounds) | best round | episodes/s |
|---|---|---|---|
| `DeviceEpisodeSampler.batch(%d)`, channel-major | %.3f | %.3f | %.0f |
| `DeviceEpisodeSampler.batch(%d)`, point-major views | %.3f | %.3f | %.0f |
| of which: %d `plan()` calls on the host | %.3f | %.3f | |
| of which: the `%s` launch with its record read | %.3f | %.3f | |
| `NoiseEpisodeSampler.episode()`, one core, blocks cached in memory | %.3f per episode | | %.0f |

How the time was taken: `batch()`, `plan()` and the host sampler by a host clock around calls that end in a device
synchronise (`batch()` reads the kernel's record back, so every call ends synchronised); 3 warm-up calls, %d calls per
round, 5 rounds.  The launch by HIP events around %d back-to-back `ops.%s` calls on resident descriptors, 5
rounds: the kernel and its record read, without planning, descriptor upload and the two dense copies `EpisodeBatch`
keeps of `support_x` / `query_x`.  No profiler attached.  The trainer's rate is what `bench.py --gpus 1` reports
(388 episodes/s in `BENCH_r04.json`).
""" % (E, args.iters, args.noise,
       "train mode, noise ratios 0 / 0.2 / 0.4" if args.noise == "train" else "test mode, %s noise at ratio 0.4" % args.noise,
       len(pool), res["pool_rows"], E * 12, E, b["mean_ms"], b["best_ms"], b["episodes_per_s"], E,
       res["batch_pm"]["mean_ms"], res["batch_pm"]["best_ms"], res["batch_pm"]["episodes_per_s"], E, res["plan"]["mean_ms"],
       res["plan"]["best_ms"], "r3d_episode_cut_partial" if partial else "r3d_episode_cut", res["launch"]["mean_ms"],
       res["launch"]["best_ms"], ms, 1e3 / ms, args.iters, args.iters, "episode_cut_partial" if partial else "episode_cut"))


if __name__ == "__main__":
    main()
