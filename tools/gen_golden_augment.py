"""Generates tests/golden/augment.npz by RUNNING the reference's own augment_pointcloud (dataloaders/loader.py:354-373) and
the XYZ lines that follow its call (loader.py:209-213) (build container only).

    python tools/gen_golden_augment.py          # needs /root/reference

TEST INFRASTRUCTURE, not imported by the package.  loader.py imports h5py, open3d and transforms3d; none is installed here.
The first two are reached by none of these calls (empty stand-in modules, as oracle/gen_golden_sampler.py).  transforms3d IS
reached: augment_pointcloud calls transforms3d.zooms.zfdir2mat and transforms3d.axangles.axangle2mat.  The stand-in module
below is NOT that package: it is written here from the published formulas --

    zfdir2mat(f, d)    = I - (1 - f) d d^T / (d^T d)         (zoom by f along direction d; no direction: f I)
    axangle2mat(n, a)  = cos a I + sin a [n]x + (1 - cos a) n n^T   (Rodrigues' rotation formula, n normalised)

-- the same situation as faiss in oracle/gen_golden_head.py.  Everything else that runs is the reference's code.

4 clouds of 250 points (x, y in [0, 1], z in [0, 3], min-shifted, float32-representable) go through two configurations on a
seeded `random` / `np.random` stream each.  Stored per configuration c<i>/: cfg (scale, rot, mirror_prob, jitter), seed, M
(4, 3, 3) and noise (4, 250, 3) float32 that the call drew, and the reference's outputs xyz, XYZ (4, 250, 3) float64;
once: x (4, 250, 3) float64 and min_extent, the smallest extent of any augmented cloud on any axis.

The reference does not return M or the noise.  They are drawn a second time here from the re-seeded streams, with the same
calls in the same order, and the script asserts that P . M^T + noise reproduces the reference's output EXACTLY -- which it
only does if these are the draws the reference made.
"""
import math
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

OUT = os.path.join(ROOT, "tests", "golden")
CONFIGS = [dict(scale=1.2, rot=1, mirror_prob=1.0, jitter=1), dict(scale=0, rot=1, mirror_prob=0, jitter=0)]
SEEDS = [31, 32]
B, N = 4, 250


def zfdir2mat(factor, direction=None):
    if direction is None:
        return np.diag([float(factor)] * 3)
    d = np.asarray(direction, np.float64)
    return np.eye(3) - (1.0 - factor) * np.outer(d, d) / np.dot(d, d)


def axangle2mat(axis, angle):
    n = np.asarray(axis, np.float64)
    n = n / math.sqrt(np.dot(n, n))
    x, y, z = n
    c, s = math.cos(angle), math.sin(angle)
    cross = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return c * np.eye(3) + s * cross + (1.0 - c) * np.outer(n, n)


def install_environment():
    for name in ("h5py", "open3d"):
        sys.modules[name] = types.ModuleType(name)
    t3d = types.ModuleType("transforms3d")
    t3d.zooms = types.ModuleType("transforms3d.zooms")
    t3d.zooms.zfdir2mat = zfdir2mat
    t3d.axangles = types.ModuleType("transforms3d.axangles")
    t3d.axangles.axangle2mat = axangle2mat
    sys.modules["transforms3d"] = t3d
    sys.modules["transforms3d.zooms"] = t3d.zooms
    sys.modules["transforms3d.axangles"] = t3d.axangles
    if not hasattr(np, "int"):
        np.int = int


def clouds():
    rs = np.random.RandomState(7)
    x = (rs.uniform(0, 1, (B, N, 3)) * np.array([1.0, 1.0, 3.0])).astype(np.float32)
    x = x - x.min(axis=1, keepdims=True)  # float32 arithmetic: the prepared clouds of the package are float32
    assert x.dtype == np.float32
    return x.astype(np.float64)


def redraw(cfg):
    """The draws of one augment_pointcloud call, from the streams as they stand (order of loader.py:356-372)."""
    M = zfdir2mat(1)
    if cfg["scale"] > 1:
        M = np.dot(zfdir2mat(random.uniform(1 / cfg["scale"], cfg["scale"])), M)
    if cfg["rot"] == 1:
        M = np.dot(axangle2mat([0, 0, 1], random.uniform(0, 2 * math.pi)), M)
    if cfg["mirror_prob"] > 0:
        if random.random() < cfg["mirror_prob"] / 2:
            M = np.dot(zfdir2mat(-1, [1, 0, 0]), M)
        if random.random() < cfg["mirror_prob"] / 2:
            M = np.dot(zfdir2mat(-1, [0, 1, 0]), M)
    noise = np.zeros((N, 3), np.float32)
    if cfg["jitter"]:
        noise = np.clip(0.01 * np.random.randn(N, 3), -0.05, 0.05).astype(np.float32)
    return M, noise


def main():
    install_environment()
    from dataloaders.loader import augment_pointcloud  # the reference
    x = clouds()
    rec = {"x": x}
    min_extent = np.inf
    for i, (cfg, seed) in enumerate(zip(CONFIGS, SEEDS)):
        random.seed(seed)
        np.random.seed(seed)
        xyz_out, XYZ_out = [], []
        for b in range(B):
            xyz = augment_pointcloud(x[b].copy(), cfg)       # loader.py:208
            xyz_min = np.amin(xyz, axis=0)                   # loader.py:210-213
            XYZ = xyz - xyz_min
            xyz_max = np.amax(XYZ, axis=0)
            XYZ = XYZ / xyz_max
            assert xyz.dtype == np.float64 and (xyz_max >= 0.5).all(), xyz_max
            min_extent = min(min_extent, float(xyz_max.min()))
            xyz_out.append(xyz)
            XYZ_out.append(XYZ)
        random.seed(seed)
        np.random.seed(seed)
        Ms, noises = zip(*[redraw(cfg) for _ in range(B)])
        for b in range(B):
            again = np.dot(x[b], Ms[b].T)
            if cfg["jitter"]:
                again = again + noises[b]
            assert np.array_equal(again, xyz_out[b]), "the re-drawn M / noise are not the reference's draws"
        pre = "c%d/" % i
        rec[pre + "cfg"] = np.array([cfg["scale"], cfg["rot"], cfg["mirror_prob"], cfg["jitter"]], np.float64)
        rec[pre + "seed"] = np.int64(seed)
        rec[pre + "M"] = np.stack(Ms)
        rec[pre + "noise"] = np.stack(noises)
        rec[pre + "xyz"] = np.stack(xyz_out)
        rec[pre + "XYZ"] = np.stack(XYZ_out)
        print("config %d %s: mirrored clouds %d of %d, |noise| max %.4f" % (
            i, cfg, sum(np.linalg.det(M) < 0 for M in Ms), B, float(np.abs(np.stack(noises)).max())))
    rec["min_extent"] = np.float64(min_extent)
    os.makedirs(OUT, exist_ok=True)
    out = os.path.join(OUT, "augment.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out), "min_extent %.4f" % min_extent)


if __name__ == "__main__":
    main()
