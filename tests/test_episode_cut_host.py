"""Cutting episodes on the device, the host side ("Cutting episodes on the device"): the numpy restatement
of the cut (tests/episode_cut_ref.py) has the properties of the definition, the planner keeps NoiseEpisodeSampler's rules,
BlockPool keeps its books, and NoiseEpisodeSampler -- whose rule code the planner now shares -- is unchanged."""
import os

import numpy as np
import pytest
import torch

import episode_cut_ref as R
from r3dfsseg_amd import _lib
from r3dfsseg_amd.block_pool import (FLAG_GT_ZERO, FLAG_QUERY, BlockPool, DeviceEpisodeSampler, EpisodePlanner, share)
from r3dfsseg_amd.episode_sampler import NoiseEpisodeSampler, SyntheticBlocks

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASSES = list(range(1, 7))
N = 512


@pytest.fixture(scope="module")
def source():
    return SyntheticBlocks(classes=CLASSES, scans_per_class=8, points_per_block=700, seed=1)


@pytest.fixture(scope="module")
def pool(source):
    return BlockPool.from_source(source, device="cpu")


def test_abi_declares_the_cut_and_stays_version_5():
    assert _lib.ABI_VERSION == 6 and "r3d_episode_cut" in _lib.header_symbols()
    res, args = _lib._SIGS["r3d_episode_cut"]
    assert res is _lib.c_i and len(args) == 27 and args[12] is _lib.c_u and args[4] is _lib.c_l


def test_draw_functions_on_known_values():
    """mix is the 32-bit finaliser of augment.hip (lowbias32); values computed by hand-running the five steps in Python ints."""
    def mix_int(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xffffffff; x ^= x >> 15; x = x * 0x846ca68b & 0xffffffff; x ^= x >> 16
        return x
    for x in (0, 1, 0xdeadbeef, 0xffffffff):
        assert int(R.mix(x)) == mix_int(x)
    s, k, i = 12345, 0xfffffffe, 1 << 20
    h = (mix_int((k * 0x9E3779B1 + s) & 0xffffffff) + s * 0x85EBCA77) & 0xffffffff
    assert int(R.stream(s, k)) == h
    assert int(R.draw(h, i)) == mix_int(h ^ ((i * 0x9E3779B1 + 0x632BE5AB) & 0xffffffff))
    assert R.draw(h, np.arange(5)).dtype == np.uint64 and int(R.draw(h, np.arange(5)).max()) < 2 ** 32


def test_restatement_properties_on_a_blocks_own_class(source, pool):
    """Every block of the source, cut for the class it is listed under."""
    small = big = 0
    least = N
    for name in pool.names:
        c = int(name[1:].split("_")[0])
        blk = source.load(name)
        lab = blk[:, 6].astype(np.int32)
        n, nv = len(lab), int((lab == c).sum())
        m_A = share(pool.count(name, c), pool.size(name), N)
        assert pool.size(name) == n and pool.count(name, c) == nv
        assert m_A == (nv if n < N else int(nv / float(n) * N))  # loader.py:227-231
        least = min(least, m_A)
        sl = R.slots(lab, N, c, m_A, seed=3, key=pool.index[name])
        assert sl.shape == (N,) and sl.min() >= 0 and sl.max() < n            # every slot in range
        a, b = sl[:m_A], sl[m_A:]
        assert np.all(lab[a] == c) and np.all(np.diff(a) > 0)                 # A: the class's points, ascending, no duplicate
        if n >= N:
            big += 1
            assert np.all(np.diff(b) > 0) and len(b) == N - m_A               # B: ascending, no duplicate
        else:
            small += 1
            assert np.array_equal(a, np.nonzero(lab == c)[0])                 # slots 0 .. nv - 1: exactly the class's points
    assert (small, big, least) == (17, 31, 71)


def test_the_index_breaks_a_tie_between_equal_draws(monkeypatch):
    monkeypatch.setattr(R, "draw", lambda h, i: np.asarray(i, np.uint64) // np.uint64(2))
    cand = np.arange(10)
    assert R.select(cand, 0, 3).tolist() == [0, 1, 2]        # draws 0 0 1 1 ...: of the two with draw 1 the lower index
    assert R.select(cand, 0, 4).tolist() == [0, 1, 2, 3]
    assert R.select(cand[::-1].copy(), 0, 5).tolist() == [0, 1, 2, 3, 4]   # whatever order the candidates come in
    labels = np.array([7, 1, 1, 7, 1, 1, 1, 7, 1, 1] * 2)
    sl = R.slots(labels, 8, 1, 3, seed=0, key=0)             # n >= N: A among the class's points, B among all
    assert sl[:3].tolist() == [1, 2, 4] and sl[3:].tolist() == [0, 1, 2, 3, 4]


def _sampler(pool, noise_type, **kw):
    cfg = dict(n_way=2, k_shot=5, n_queries=1, num_point=N, seed=7)  # (the reference's 5-shot: at 4 shots and 2 noisy
    # ones its own retiring rule empties a 2-way 'sym' range and its re-draw loop never ends)
    if noise_type == "train":
        cfg.update(mode="train", noise_ratio=[0.4])
    else:
        cfg.update(mode="test", noise_type=noise_type, noise_ratio=0.4,
                   noise_pair_dict={c: c % 6 + 1 for c in CLASSES} if noise_type == "pair" else None)
    cfg.update(kw)
    return DeviceEpisodeSampler(pool, CLASSES, **cfg)


@pytest.mark.parametrize("noise_type", ["train", "sym", "ood", "pair"])
def test_plan_rules(pool, noise_type):
    s = _sampler(pool, noise_type)
    n_way, k_shot, S = 2, 5, 10
    saw_noise_from = set()
    for _ in range(6):
        p = s.plan()
        d, sc, flag = p.desc, p.sampled_classes.tolist(), p.support_flag
        assert d.shape == (S + 1 * n_way, 5) and d.dtype == np.int32 and flag.shape == (n_way, k_shot)
        assert len(set(d[:, 0].tolist())) == len(d)                          # no block twice in an episode
        assert sorted(pool.names[b] for b in d[:, 0]) == sorted(str(x) for x in s.planner.last_black_list)
        assert np.all((d[:S, 3] & FLAG_QUERY) == 0) and np.all(d[S:, 3] == FLAG_QUERY)
        for w, cls in enumerate(sc):
            rows = d[w * k_shot:(w + 1) * k_shot]
            noisy = (rows[:, 3] & FLAG_GT_ZERO) != 0
            assert int(noisy.sum()) == int(round(k_shot * 0.4))              # the noisy-shot count
            assert np.array_equal(rows[:, 1], flag[w])                       # flags line up with the shots after the shuffle
            assert np.array_equal(noisy, flag[w] != cls)                     # and so do the gt-zero bits
            assert np.all(rows[~noisy, 1] == cls)
            for c in rows[noisy, 1].tolist():
                saw_noise_from.add(c)
                if noise_type == "sym":
                    assert c in sc and c != cls
                elif noise_type == "ood":
                    assert c not in sc
                elif noise_type == "pair":
                    assert c == cls % 6 + 1
                else:
                    assert c != cls and c in CLASSES
            for b, c, m_A, _, _ in rows.tolist():                             # the block is listed under the shot's class
                assert pool.names[b] in pool.class2scans[c]
                assert m_A == share(pool.count(b, c), pool.size(b), N) > 0
        for j, cls in enumerate(sc):                                         # queries: one per way, of the way's class
            assert d[S + j, 1] == cls and pool.names[d[S + j, 0]] in pool.class2scans[cls]
        k0 = p.keyed(5)[:, 4]
        assert np.array_equal(k0, 5 * len(d) + np.arange(len(d)))            # key = counter (S + Q) + i
    assert len(saw_noise_from) > 1


def test_plan_draws_the_host_samplers_stream_until_the_first_cloud(pool, source):
    """Same seed, same classes and, for a clean episode, the same first way's blocks: the planner takes the plan draws
    from the stream the host sampler uses, in its order (the clouds' own draws are what it leaves out)."""
    kw = dict(n_way=2, k_shot=2, n_queries=1, num_point=N, mode="test", noise_ratio=0.0, noise_type="sym", seed=11)
    host, plan = NoiseEpisodeSampler(source, CLASSES, **kw), EpisodePlanner(pool, CLASSES, **kw)
    _, sc = host.episode()
    p = plan.plan()
    assert np.array_equal(sc, p.sampled_classes)
    first_way = [pool.names[b] for b in [p.desc[4, 0]] + p.desc[0:2, 0].tolist()]  # query, then the shots
    assert sorted(first_way) == sorted(str(x) for x in host.last_black_list[:3])


def test_partial_noise_is_refused_and_names_the_host_sampler(pool):
    with pytest.raises(NotImplementedError, match="NoiseEpisodeSampler"):
        _sampler(pool, "partial")
    with pytest.raises(ValueError, match="pc_attribs"):
        _sampler(pool, "sym", pc_attribs="rgb")


class _Hand:
    """A hand-made source: blocks[name] = rows, class2scans given."""

    def __init__(self, blocks, class2scans):
        self.blocks, self.class2scans = blocks, class2scans

    def load(self, name):
        return self.blocks[name]


def _rows(n, labels, seed=0):
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 8))
    out[:, :3] = rs.uniform(0, 2, (n, 3))
    out[:, 3:6] = rs.randint(0, 256, (n, 3))
    out[:, 6] = labels
    return out


def test_a_support_block_whose_share_is_zero_raises_before_any_launch():
    """3 of 2000 points: int(3 / 2000 * 512) = 0, an empty mask (the reference asserts against it, loader.py:350)."""
    blocks, c2s = {}, {1: [], 2: []}
    for c in (1, 2):
        for i in range(3):
            lab = np.zeros(2000)
            lab[:3] = c
            blocks["b%d_%d" % (c, i)] = _rows(2000, lab, seed=10 * c + i)
            c2s[c].append("b%d_%d" % (c, i))
    pool = BlockPool.from_source(_Hand(blocks, c2s), device="cpu")
    s = DeviceEpisodeSampler(pool, [1, 2], n_way=1, k_shot=2, n_queries=1, num_point=N, mode="test", noise_ratio=0.0, seed=0)
    with pytest.raises(ValueError, match=r"block b1_\d keeps no point of class 1"):
        s.plan(sampled_classes=[1])


def test_a_host_pool_plans_but_does_not_cut(pool):
    s = _sampler(pool, "sym")
    with pytest.raises(RuntimeError, match="HIP kernel"):
        s.cut([s.plan()], 0)  # no host fall-back: NoiseEpisodeSampler is the host sampler


def test_block_pool_books(source, pool):
    assert pool.names == [n for c in CLASSES for n in source.class2scans[c]] and len(pool) == 48
    assert pool.points.dtype == torch.float32 and pool.labels.dtype == torch.int32 and pool.offsets.dtype == torch.int64
    assert not pool.points.is_cuda and pool.points.shape == (int(pool.offsets[-1]), 6) and pool.labels.shape == (pool.points.shape[0],)
    off = pool.offsets.numpy()
    assert off[0] == 0 and len(off) == 49
    for name in ("c1_0", "c3_5", "c6_7"):
        b = pool.index[name]
        blk = source.load(name)
        assert pool.names[b] == name and off[b + 1] - off[b] == len(blk) == pool.size(b)
        assert np.array_equal(pool.points[off[b]:off[b + 1]].numpy(), blk[:, :6].astype(np.float32))
        assert np.array_equal(pool.labels[off[b]:off[b + 1]].numpy(), blk[:, 6].astype(np.int32))
        for c in range(0, 8):
            assert pool.count(b, c) == pool.count(name, c) == int((blk[:, 6] == c).sum())
    assert pool.class2scans == {c: list(v) for c, v in source.class2scans.items()}
    sub = BlockPool.from_source(source, names=["c2_1", "c1_0", "c2_3"], device="cpu")
    assert sub.names == ["c2_1", "c1_0", "c2_3"] and sub.index["c1_0"] == 1
    assert sub.class2scans[2] == ["c2_1", "c2_3"] and sub.class2scans[1] == ["c1_0"] and sub.class2scans[5] == []


def test_block_pool_limits():
    ok = _rows(5, [1, 1, 2, 0, 0])
    for bad, what in (({"a": _rows(5, [1, 1, 2, 0, 2.0 ** 31])}, "int32"),
                      ({"a": _rows(5, [1, 1, 2, 0, 0.5])}, "int32"),
                      ({"a": np.zeros((0, 8))}, "0 points"),
                      ({"a": ok[:, :6]}, "shape")):
        with pytest.raises(ValueError, match=what):
            BlockPool.from_source(_Hand(bad, {1: ["a"]}), device="cpu")
    with pytest.raises(ValueError, match="names"):
        BlockPool.from_source(_Hand({"a": ok}, {1: ["a"]}), names=["a", "a"], device="cpu")

    class Huge:
        """(2^20 + 1, 7) rows without the memory: a broadcast view."""
        class2scans = {1: ["h"]}

        def load(self, name):
            return np.broadcast_to(np.zeros((1, 7)), ((1 << 20) + 1, 7))
    with pytest.raises(ValueError, match=r"2\^20"):
        BlockPool.from_source(Huge(), device="cpu")
    one = BlockPool.from_source(_Hand({"a": ok[:1]}, {1: ["a"]}), device="cpu")  # one point is a block
    assert one.size("a") == 1 and one.count("a", 1) == 1


def test_noise_episode_sampler_is_what_the_parent_commit_computed(source):
    """tests/golden/noise_episode_sampler_parent.npz holds one episode per scenario as the commit BEFORE the rule code moved
    into episode_rules produced it (the project's own data): there, with the source of this module,
        for tag, kw in (("train", dict(mode="train", noise_ratio=[0.5])),
                        ("pair", dict(mode="test", noise_type="pair", noise_ratio=0.5, noise_pair_dict={c: c % 6 + 1 ...}))):
            s = NoiseEpisodeSampler(source, [1 .. 6], n_way=2, k_shot=2, n_queries=1, num_point=128, seed=5, **kw)
            arrays, _ = s.episode();  out[tag + "/%d" % i] = arrays[i];  out[tag + "/after"] = s.rng.randint(0, 2**31 - 1, 4)
        np.savez_compressed(path, **out)
    Equal arrays and an equal next draw: same behaviour, same random stream."""
    g = np.load(os.path.join(GOLD, "noise_episode_sampler_parent.npz"))
    for tag, kw in (("train", dict(mode="train", noise_ratio=[0.5])),
                    ("pair", dict(mode="test", noise_type="pair", noise_ratio=0.5, noise_pair_dict={c: c % 6 + 1 for c in CLASSES}))):
        s = NoiseEpisodeSampler(source, CLASSES, n_way=2, k_shot=2, n_queries=1, num_point=128, seed=5, **kw)
        arrays, _ = s.episode()
        assert len(arrays) == (12 if tag == "train" else 8)
        for i, a in enumerate(arrays):
            w = g["%s/%d" % (tag, i)]
            assert a.dtype == w.dtype and a.shape == w.shape and np.array_equal(a, w), (tag, i)
        assert np.array_equal(s.rng.randint(0, 2 ** 31 - 1, 4), g[tag + "/after"]), tag
