"""Partial noise in the device episode sampler, the host side ("Cutting episodes on the device", steps
P0-P7): the ABI declares the new entry point, BlockPool keeps instance ids and the books the planner's "poor block" test
reads, the planner keeps NoiseEpisodeSampler's rules for noise_type="partial", the numpy restatement of the mask edit
(tests/episode_partial_ref.py) has the properties and the distribution of the definition, and NoiseEpisodeSampler is
unchanged by the hook the planner passes into episode_rules."""
import numpy as np
import pytest
import torch

import episode_cut_ref as R
import episode_partial_ref as P
from r3dfsseg_amd import _lib, episode_sampler
from r3dfsseg_amd.block_pool import (FLAG_GT_ZERO, FLAG_PARTIAL, FLAG_QUERY, BlockPool, DeviceEpisodeSampler, EpisodePlanner)
from r3dfsseg_amd.episode_sampler import NoiseEpisodeSampler, SyntheticBlocks

CLASSES = list(range(1, 7))
N = 512


@pytest.fixture(scope="module")
def source():
    return SyntheticBlocks(classes=CLASSES, scans_per_class=8, points_per_block=700, seed=1)


@pytest.fixture(scope="module")
def pool(source):
    return BlockPool.from_source(source, device="cpu", instances=True)


class _Hand:
    def __init__(self, blocks, class2scans):
        self.blocks, self.class2scans = blocks, class2scans

    def load(self, name):
        return self.blocks[name]


def _rows(labels, inst, seed=0):
    n = len(labels)
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 8))
    out[:, :3] = rs.uniform(0, 2, (n, 3))
    out[:, 3:6] = rs.randint(0, 256, (n, 3))
    out[:, 6] = labels
    out[:, 7] = inst
    return out


def test_abi_declares_the_partial_cut_and_stays_version_5():
    assert _lib.ABI_VERSION == 6 and "r3d_episode_cut_partial" in _lib.header_symbols()
    res, args = _lib._SIGS["r3d_episode_cut_partial"]
    old = _lib._SIGS["r3d_episode_cut"][1]
    assert res is _lib.c_i and len(old) == 27 and len(args) == 29
    assert args[:26] == old[:26] and args[26] is _lib.c_f and args[27] is _lib.c_f and args[28] is old[26]


def test_pool_books_with_instances(source, pool):
    plain = BlockPool.from_source(source, device="cpu")
    assert plain.instances is None and plain.n_objects is None and plain.n_classes is None
    assert torch.equal(plain.points, pool.points) and torch.equal(plain.labels, pool.labels) and torch.equal(plain.offsets, pool.offsets)
    assert pool.instances.dtype == torch.int32 and pool.instances.shape == pool.labels.shape and not pool.instances.is_cuda
    assert len(pool.n_objects) == len(pool.n_classes) == len(pool) == 48
    off = pool.offsets.numpy()
    for name in ("c1_0", "c3_5", "c6_7"):
        b = pool.index[name]
        blk = source.load(name)
        assert np.array_equal(pool.instances[off[b]:off[b + 1]].numpy(), blk[:, -1].astype(np.int32))
        assert pool.n_objects[b] == len(np.unique(blk[:, -1])) and pool.n_classes[b] == len(np.unique(blk[:, 6]))
    wide = np.concatenate([_rows([1, 1, 2], [9, 9, 9]), np.array([[5.0], [-6.0], [5.0]])], 1)  # the LAST column, as data[:, -1]
    p = BlockPool.from_source(_Hand({"a": wide}, {1: ["a"]}), device="cpu", instances=True)
    assert p.instances.tolist() == [5, -6, 5] and p.n_objects.tolist() == [2] and p.n_classes.tolist() == [2]
    edge = _rows([1, 1, 2, 2], [-2 ** 31, 2 ** 31 - 1, 0, -1])
    p = BlockPool.from_source(_Hand({"a": edge}, {1: ["a"]}), device="cpu", instances=True)
    assert p.instances.tolist() == [-2 ** 31, 2 ** 31 - 1, 0, -1] and p.n_objects.tolist() == [4]


def test_pool_instance_limits():
    ok = _rows([1, 1, 2, 0, 0], [1, 1, 2, 0, 0])
    for bad, what in (({"a": ok[:, :7]}, "shape"),
                      ({"a": _rows([1, 1, 2, 0, 0], [1, 1, 2, 0, 0.5])}, "instance id that is not an int32"),
                      ({"a": _rows([1, 1, 2, 0, 0], [1, 1, 2, 0, 2.0 ** 31])}, "instance id that is not an int32")):
        with pytest.raises(ValueError, match=what):
            BlockPool.from_source(_Hand(bad, {1: ["a"]}), device="cpu", instances=True)
    assert BlockPool.from_source(_Hand({"a": ok[:, :7]}, {1: ["a"]}), device="cpu").instances is None  # 7 columns do without


def test_plan_rules_for_partial_noise(pool):
    s = DeviceEpisodeSampler(pool, CLASSES, n_way=2, k_shot=5, n_queries=1, num_point=N, seed=7, mode="test",
                             noise_type="partial", noise_ratio=0.4)
    n_way, k_shot, S = 2, 5, 10
    for _ in range(6):
        p = s.plan()
        d, sc, flag = p.desc, p.sampled_classes.tolist(), p.support_flag
        assert d.shape == (S + n_way, 5) and d.dtype == np.int32 and flag.shape == (n_way, k_shot)
        assert len(set(d[:, 0].tolist())) == len(d)                          # no block twice in an episode
        assert sorted(pool.names[b] for b in d[:, 0]) == sorted(str(x) for x in s.planner.last_black_list)
        assert np.all(d[S:, 3] == FLAG_QUERY)
        for w, cls in enumerate(sc):
            rows = d[w * k_shot:(w + 1) * k_shot]
            noisy = (rows[:, 3] & FLAG_PARTIAL) != 0
            assert int(noisy.sum()) == int(round(k_shot * 0.4))              # the noisy-shot count
            assert np.all(rows[:, 1] == cls) and np.all(flag[w] == cls)      # the way's OWN class, and support_flag says so
            assert FLAG_PARTIAL | FLAG_GT_ZERO == 6 and np.all(rows[noisy, 3] == 6) and np.all(rows[noisy, 2] == 0)
            assert np.all(rows[~noisy, 3] == 0) and np.all(rows[~noisy, 2] > 0)  # clean shots are what they are today
            for b in rows[:, 0].tolist():
                assert pool.names[b] in pool.class2scans[cls]
        s.check(p.keyed(0))
    bad = p.keyed(0)
    bad[0, 2], bad[0, 3] = 3, 6
    with pytest.raises(ValueError, match="cloud 0: flags 6"):                # P0 on the host, before any launch
        s.check(bad)
    bad = p.keyed(0)
    bad[S, 3] = FLAG_QUERY | FLAG_PARTIAL
    with pytest.raises(ValueError, match="cloud %d: flags 5" % S):
        s.check(bad)
    sym = DeviceEpisodeSampler(pool, CLASSES, n_way=2, k_shot=5, n_queries=1, num_point=N, seed=7, mode="test",
                               noise_type="sym", noise_ratio=0.4)
    bad = p.keyed(0)
    with pytest.raises(ValueError, match="partial"):                         # the plain entry point would refuse bit 2
        sym.check(bad)


def test_a_pool_without_instances_still_refuses():
    src = SyntheticBlocks(classes=CLASSES, scans_per_class=8, points_per_block=700, seed=1)
    plain = BlockPool.from_source(src, device="cpu")
    with pytest.raises(NotImplementedError, match=r"instances=True.*NoiseEpisodeSampler"):
        EpisodePlanner(plain, CLASSES, noise_type="partial")


def _poor_source(rich_per_class):
    """12 blocks per class: `rich_per_class` with 3 objects of 3 classes, the others poor in turn (2 objects / 2 classes)."""
    blocks, c2s = {}, {1: [], 2: []}
    for c in (1, 2):
        for i in range(12):
            n = 60
            if i < rich_per_class:
                lab = np.repeat([c, 3 - c, 0], n // 3)
                inst = np.repeat([1, 2, 3], n // 3)
            elif i % 2:
                lab = np.repeat([c, 3 - c, 0], n // 3)   # 3 classes, 2 objects
                inst = np.repeat([1, 2, 2], n // 3)
            else:
                lab = np.repeat([c, 0, 0], n // 3)       # 3 objects, 2 classes
                inst = np.repeat([1, 2, 3], n // 3)
            name = "b%d_%d" % (c, i)
            blocks[name] = _rows(lab, inst, seed=20 * c + i)
            c2s[c].append(name)
    return _Hand(blocks, c2s)


def test_poor_blocks_are_never_planned_as_noisy_shots():
    src = _poor_source(6)
    pool = BlockPool.from_source(src, device="cpu", instances=True)
    assert sorted(set(pool.n_objects.tolist())) == [2, 3] and sorted(set(pool.n_classes.tolist())) == [2, 3]
    poor = {n for n in pool.names if int(n.split("_")[1]) >= 6}
    p = EpisodePlanner(pool, [1, 2], n_way=2, k_shot=5, n_queries=1, num_point=32, mode="test", noise_type="partial",
                       noise_ratio=0.4, seed=3)
    noisy_blocks, clean_poor = set(), 0
    for _ in range(50):
        d = p.plan().desc
        for b, _, _, flags, _ in d.tolist():
            if flags & FLAG_PARTIAL:
                assert pool.names[b] not in poor
                noisy_blocks.add(pool.names[b])
            else:
                clean_poor += pool.names[b] in poor
    assert len(noisy_blocks) > 6 and clean_poor > 0  # the test is for noisy shots alone: clean ones may be poor


def test_all_poor_candidates_raise_instead_of_looping():
    pool = BlockPool.from_source(_poor_source(0), device="cpu", instances=True)
    p = EpisodePlanner(pool, [1, 2], n_way=2, k_shot=5, n_queries=1, num_point=32, mode="test", noise_type="partial",
                       noise_ratio=0.4, seed=3)
    with pytest.raises(ValueError, match=r"class [12]: every one of its 8 unused blocks"):
        p.plan()


def _dids(lab, inst, c, keys, seed=0):
    return np.array([P.edit(lab, inst, c, seed, k)[2] for k in keys])


def test_restatement_flip_rules():
    keys = range(200)
    c = 5
    one = _dids(np.repeat([5, 7], 20), np.full(40, 3), c, keys)               # one object only: K == 1, never a flip
    assert np.all(one[:, 0] == 1) and not (one[:, 3] & 1).any()
    same = _dids(np.full(40, 5), np.repeat([3, 4], 20), c, keys)              # two objects of one class: not `multi`
    assert np.all(same[:, 0] == 2) and not (same[:, 3] & 1).any()
    other = _dids(np.full(40, 7), np.repeat([3, 4], 20), c, keys)             # ... of another class: eligible, still not multi
    assert np.all(other[:, 1] == 2) and not (other[:, 3] & 1).any() and np.all(other[:, 3] == 0)
    # object 8: its lowest slot has label c, its later slots do not -> not eligible; objects 2 and 9 are
    lab = np.array([7] * 10 + [5] + [7] * 9 + [5] * 10 + [0] * 10)
    inst = np.array([2] * 10 + [8] * 10 + [1] * 10 + [9] * 10)
    d = _dids(lab, inst, c, keys)
    assert np.all(d[:, 0] == 4) and np.all(d[:, 1] == 2) and np.all(d[:, 2] == 2)   # K, e (2 and 9), f (8 and 1)
    assert np.all(d[:, 3] & 1) and set(d[:, 4].tolist()) == {2, 9} and np.all(d[:, 5] == 10)
    for k in keys:                                                           # the flipped object never has `first` label c
        m0, m, rec = P.edit(lab, inst, c, 0, k)
        first = np.nonzero(inst == rec[4])[0][0]
        assert lab[first] != c and np.array_equal(m0, lab == c)
        want = m0 | (inst == rec[4])
        if rec[3] & 2:
            want = want & ~(inst == rec[6])
            assert rec[6] in (8, 1) and rec[7] == 10
        else:
            assert rec[6] == 0 and rec[7] == 0
        assert np.array_equal(m, want)
    signed = _dids(np.array([7, 5, 0, 7]), np.array([2 ** 31 - 1, -2 ** 31, -1, 0]), c, range(400))   # ascending as SIGNED
    assert set(signed[:, 4].tolist()) == {-1, 0, 2 ** 31 - 1} and np.all(signed[:, 1] == 3)


def test_the_drop_is_skipped_exactly_when_it_would_empty_the_mask():
    c, seed = 5, 11
    alone = (np.full(30, 5), np.full(30, 4))                                   # one object, all of class c: no flip, f == 1
    two = (np.array([5] * 10 + [7] * 20), np.array([1] * 10 + [2] * 20))       # a flip always: the mask survives any drop
    split = (np.array([5] * 10 + [5] * 10 + [5] * 10), np.array([1] * 10 + [2] * 10 + [3] * 10))  # no flip, f == 3: it survives
    drawn_key = skipped = applied = None
    for key in range(300):
        drawn = int(R.draw(R.stream(seed, 2 * key), 1)) > 0xB3333333
        for lab, inst in (alone, two, split):
            m0, m, rec = P.edit(lab, inst, c, seed, key)
            flip = bool(rec[3] & 1)
            m1 = m0 | (inst == rec[4]) if flip else m0
            if not drawn:
                assert rec[3] & 6 == 0 and np.array_equal(m, m1)
                continue
            r2 = (int(R.draw(R.stream(seed, 2 * key), 2)) * int(rec[2])) >> 32
            o = np.unique(inst[m0])[r2]
            left = m1 & ~(inst == o)
            if left.any():
                assert rec[3] & 6 == 2 and rec[6] == o and rec[7] == (inst == o).sum() and np.array_equal(m, left)
                applied = key
            else:
                assert rec[3] & 6 == 4 and rec[6] == 0 and rec[7] == 0 and np.array_equal(m, m1) and m.any()
                skipped = key
                assert lab is alone[0]
    assert skipped is not None and applied is not None


def test_distribution_of_drop_and_flip(source):
    """4000 keys of one block: the drop is drawn in a share within 4 binomial standard deviations of 0.3 (+- 0.029); each
    of the block's e eligible objects is flipped in a share within 4 standard deviations of 1 / e."""
    blk = source.load("c2_3")
    lab, inst = blk[:, 6].astype(np.int32), blk[:, 7].astype(np.int32)
    c, seed, n = 2, 5, 4000
    rec = np.array([P.edit(lab[sl], inst[sl], c, seed, k)[2] for k in range(n)
                    for sl in [R.slots(lab, N, c, 0, seed, k)]])
    e = int(rec[0, 1])
    assert e >= 2 and np.all(rec[:, 1] == e) and np.all(rec[:, 2] >= 1) and np.all(rec[:, 3] & 1)  # every key: same objects, a flip
    drawn = ((rec[:, 3] & 6) != 0).mean()
    assert abs(drawn - 0.3) <= 4 * np.sqrt(0.3 * 0.7 / n) < 0.029, drawn
    objs, cnt = np.unique(rec[:, 4], return_counts=True)
    assert len(objs) == e
    sd = np.sqrt((1.0 / e) * (1 - 1.0 / e) / n)
    for o, k in zip(objs, cnt):
        assert abs(k / n - 1.0 / e) <= 4 * sd, (o, k / n, e)


def test_noise_episode_sampler_partial_is_unchanged_by_the_hook(source, monkeypatch):
    kw = dict(n_way=2, k_shot=5, n_queries=1, num_point=128, mode="test", noise_type="partial", noise_ratio=0.4, seed=9)
    a, b = NoiseEpisodeSampler(source, CLASSES, **kw), NoiseEpisodeSampler(source, CLASSES, **kw)
    xa, sca = a.episode()
    xb, scb = b.episode()
    assert np.array_equal(sca, scb) and a.last_black_list == b.last_black_list and len(a.last_black_list) == 12 + 4
    assert all(np.array_equal(u, v) for u, v in zip(xa, xb))
    # the hook's default is no hook: a sampler that passes one which does nothing draws and lists the same
    rules, seen = episode_sampler.episode_rules, []
    monkeypatch.setattr(episode_sampler, "episode_rules",
                        lambda *args: rules(*args, stuck=lambda cls, cand: seen.append((cls, len(cand)))))
    h = NoiseEpisodeSampler(source, CLASSES, **kw)
    xh, _ = h.episode()
    assert len(seen) == 4 and h.last_black_list == a.last_black_list and all(np.array_equal(u, v) for u, v in zip(xa, xh))
    assert np.array_equal(h.rng.randint(0, 2 ** 31 - 1, 4), a.rng.randint(0, 2 ** 31 - 1, 4))
