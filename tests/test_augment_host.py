"""Host side of --pc_augm (dataloaders/loader.py:205-213,354-373): episode_sampler.augment_pointcloud against the outputs of the
reference's own function (tests/golden/augment.npz, written by tools/gen_golden_augment.py), and its place in the sampler."""
import os
import random

import numpy as np

from r3dfsseg_amd import episode_sampler as ES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")


def _cfg(v):
    return {"scale": float(v[0]), "rot": int(v[1]), "mirror_prob": float(v[2]), "jitter": int(v[3])}


def test_augment_pointcloud_reproduces_the_reference():
    """Same seeds, same streams, same formulas, float64 on both sides: M, noise, xyz' and XYZ' to 1e-12 (the noise, a float32
    array drawn from the same numpy stream, exactly)."""
    g = np.load(GOLDEN)
    x = g["x"]
    assert x.shape == (4, 250, 3) and np.array_equal(x, x.astype(np.float32).astype(np.float64))
    for i in range(2):
        pre = "c%d/" % i
        cfg, seed = _cfg(g[pre + "cfg"]), int(g[pre + "seed"])
        pyrng, rng = random.Random(seed), np.random.RandomState(seed)
        for b in range(x.shape[0]):
            inp = x[b].copy()
            xyz, M, noise = ES.augment_pointcloud(inp, cfg, pyrng, rng, return_draws=True)
            assert np.array_equal(inp, x[b])  # the input is left alone
            assert np.abs(M - g[pre + "M"][b]).max() <= 1e-12
            assert noise.dtype == np.float32 and np.array_equal(noise, g[pre + "noise"][b])
            assert np.abs(xyz - g[pre + "xyz"][b]).max() <= 1e-12
            XYZ = xyz - np.amin(xyz, axis=0)
            XYZ = XYZ / np.amax(XYZ, axis=0)
            assert np.abs(XYZ - g[pre + "XYZ"][b]).max() <= 1e-12
    assert float(g["min_extent"]) >= 0.5


def test_augment_matrix_closed_forms():
    """What each switch contributes: nothing drawn when everything is off, s I for the scale, a z-rotation, the mirrors."""
    off = {"scale": 0, "rot": 0, "mirror_prob": 0, "jitter": 0}
    pyrng = random.Random(3)
    state = pyrng.getstate()
    assert np.array_equal(ES.augment_matrix(off, pyrng), np.eye(3)) and pyrng.getstate() == state
    M = ES.augment_matrix(dict(off, scale=1.5), random.Random(3))
    s = M[0, 0]
    assert 1 / 1.5 <= s <= 1.5 and np.array_equal(M, s * np.eye(3))
    M = ES.augment_matrix(dict(off, rot=1), random.Random(3))
    assert np.allclose(M.T @ M, np.eye(3), atol=1e-15) and np.array_equal(M[2], [0, 0, 1]) and np.linalg.det(M) > 0
    M = ES.augment_matrix(dict(off, mirror_prob=2), random.Random(3))  # probability 2 / 2: both mirrors, always
    assert np.array_equal(M, np.diag([-1.0, -1.0, 1.0]))
    x = np.random.RandomState(0).rand(50, 3)
    y = ES.augment_pointcloud(x, dict(off, jitter=1), random.Random(0), np.random.RandomState(1))
    assert 0 < np.abs(y - x).max() <= 0.05


def _block():
    return ES.SyntheticBlocks(classes=list(range(6)), scans_per_class=4, points_per_block=900, seed=5).load("c2_1")


def test_sample_pointcloud_augments_between_min_shift_and_XYZ():
    """sample_pointcloud(pc_augm=True) == the index draws, min-shift -> augment_pointcloud -> XYZ composed by hand on the same
    streams (loader.py:201-219); labels are those of the un-augmented call."""
    cfg = {"scale": 1.2, "rot": 1, "mirror_prob": 1.0, "jitter": 1}
    blk = _block()
    for support in (True, False):
        got, lab, gt = ES.sample_pointcloud(blk, 256, [2, 4], 2, support, np.random.RandomState(9), pyrng=random.Random(9),
                                            pc_augm=True, pc_augm_config=cfg)
        plain, lab0, gt0 = ES.sample_pointcloud(blk, 256, [2, 4], 2, support, np.random.RandomState(9), pyrng=random.Random(9))
        rng, pyrng = np.random.RandomState(9), random.Random(9)
        ES.sample_pointcloud(blk, 256, [2, 4], 2, support, rng)  # consumes this cloud's index draws
        xyz = ES.augment_pointcloud(plain[:, 0:3], cfg, pyrng, rng)  # plain xyz IS the min-shifted xyz
        XYZ = xyz - np.amin(xyz, axis=0)
        want = np.concatenate([xyz, plain[:, 3:6], XYZ / np.amax(XYZ, axis=0)], axis=1)
        assert got.shape == (256, 9) and np.array_equal(got, want)
        assert np.array_equal(lab, lab0) and np.array_equal(gt, gt0)
        assert not np.array_equal(got[:, 0:3], plain[:, 0:3])
        assert got[:, 6:9].min() == 0.0 and got[:, 6:9].max() == 1.0


def test_sampler_default_is_unchanged_and_switch_augments_every_cloud():
    """NoiseEpisodeSampler(pc_augm=False) gives the arrays it gives without the argument; with pc_augm every cloud of the
    episode moves (support, query and background: loader.py:701-875 hands the flag to every sample_K_pointclouds call),
    and masks / labels stay what they were for a configuration that draws nothing from the numpy stream."""
    src = ES.SyntheticBlocks(classes=list(range(8)), scans_per_class=8, points_per_block=900, seed=2)
    kw = dict(n_way=2, k_shot=3, n_queries=1, num_point=256, mode="train", noise_ratio=[0.0, 0.34], seed=4)
    base, sc0 = ES.NoiseEpisodeSampler(src, list(range(8)), **kw).episode()
    off, sc1 = ES.NoiseEpisodeSampler(src, list(range(8)), pc_augm=False, pc_augm_config=None, **kw).episode()
    assert np.array_equal(sc0, sc1) and len(base) == len(off) == 12
    for a, b in zip(base, off):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    cfg = {"scale": 1.2, "rot": 1, "mirror_prob": 1.0, "jitter": 0}  # python-stream draws only: the block choices stay
    on, sc2 = ES.NoiseEpisodeSampler(src, list(range(8)), pc_augm=True, pc_augm_config=cfg, **kw).episode()
    assert np.array_equal(sc0, sc2)
    for i in (1, 3, 7, 8, 10, 11):
        assert np.array_equal(base[i], on[i])
    for i in (0, 2, 9):
        a, b = base[i].reshape(-1, 256, 9), on[i].reshape(-1, 256, 9)
        assert len(a) and all(not np.array_equal(p[:, 0:3], q[:, 0:3]) for p, q in zip(a, b))
        assert np.array_equal(a[:, :, 3:6], b[:, :, 3:6])
        assert np.allclose(b[:, :, 6:9].min(axis=1), 0) and np.allclose(b[:, :, 6:9].max(axis=1), 1)
