"""r3d_episode_cut_partial against its numpy restatement (tests/episode_partial_ref.py), bit for bit, and the
DeviceEpisodeSampler with noise_type="partial" on top of it ("Cutting episodes on the device", steps
P0-P7).  N = 512 and blocks of 200 to 1200 points unless a case says otherwise; the hand-made cases are one cloud each."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import episode_cut_ref as R
import episode_partial_ref as P
from r3dfsseg_amd import ops, synthetic as S
from r3dfsseg_amd.block_pool import ATTRIB_SETS, BlockPool, DeviceEpisodeSampler
from r3dfsseg_amd.episode_sampler import SyntheticBlocks

pytestmark = pytest.mark.gpu

CLASSES = list(range(1, 7))
N = 512
SHAPE = dict(n_way=2, k_shot=5, n_queries=1, num_point=N)
PARTIAL = dict(mode="test", noise_type="partial", noise_ratio=0.4)
KEYS = ("x", "mask", "gt_mask", "query_y", "gt_query_y", "slot_map", "info")
I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module")
def pool():
    return BlockPool.from_source(SyntheticBlocks(classes=CLASSES, scans_per_class=8, points_per_block=700, seed=1),
                                 instances=True)


def _host(pool):
    return pool.points.cpu().numpy(), pool.labels.cpu().numpy(), pool.instances.cpu().numpy(), pool.offsets.cpu().numpy()


def _ref(pool, desc, classes, Sn, Q, seed, attribs="xyzrgbXYZ", n=N, instances=True):
    pts, lab, inst, off = _host(pool)
    return P.cut_batch_partial(pts, lab, inst if instances else None, off, desc, classes, Sn, Q, n, seed, attribs)


def _keyed(plans, counter):
    return np.concatenate([p.keyed(counter + e) for e, p in enumerate(plans)])


def _raw(pool, desc, classes, Sn, Q, seed, n=N, fill=None, instances=True, partial=True, layout="cm"):
    """ops.episode_cut_partial (or ops.episode_cut) on tensors of the test's own -> dict of tensors, error."""
    dev = pool.device
    C, rgb_ch, XYZ_ch = ATTRIB_SETS["xyzrgbXYZ"]
    classes = np.asarray(classes, np.int32)
    E = classes.shape[0]
    B = E * (Sn + Q)
    mk = (lambda *s, dt: torch.empty(*s, device=dev, dtype=dt)) if fill is None else \
        (lambda *s, dt: torch.full(s, fill, device=dev, dtype=dt))
    x = mk(B, n, C, dt=torch.float32).transpose(1, 2) if layout == "pm" else mk(B, C, n, dt=torch.float32)
    out = dict(x=x, mask=mk(E * Sn, n, dt=torch.int32), gt_mask=mk(E * Sn, n, dt=torch.int32),
               query_y=mk(E * Q, n, dt=torch.int64), gt_query_y=mk(E * Q, n, dt=torch.int64), slot_map=mk(B, n, dt=torch.int32))
    args = (pool.points, pool.labels, pool.offsets, torch.from_numpy(np.ascontiguousarray(desc, np.int32)).to(dev),
            torch.from_numpy(classes).to(dev), Sn, Q, n, seed, x, rgb_ch, XYZ_ch, out["mask"], out["gt_mask"], out["query_y"],
            out["gt_query_y"], out["slot_map"])
    err = None
    try:
        if partial:
            out["info"] = mk(B, 8, dt=torch.int32)
            ops.episode_cut_partial(*args, pool.instances if instances else None, out["info"])
        else:
            ops.episode_cut(*args)
    except ValueError as e:
        err = e
    return out, err


def _equal(got, want, what=""):
    for k, w in want.items():
        g = got[k].cpu()
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape)
        assert torch.equal(g, w), (what, k)


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_partial_batch_equals_the_restatement_bit_for_bit(pool, layout):
    s = DeviceEpisodeSampler(pool, CLASSES, seed=4, layout=layout, **SHAPE, **PARTIAL)
    b = s.batch(3)
    assert s.counter == 3 and b.E == 3
    desc = _keyed(b.plans, 0)
    sizes = np.array([pool.size(k) for k in desc[:, 0]])
    assert (sizes < N).any() and (sizes >= N).any()
    noisy = (desc[:, 3] & 4) != 0
    assert noisy.sum() == 3 * 2 * 2 and np.all(desc[noisy, 3] == 6) and np.all(desc[noisy, 2] == 0)
    want = _ref(pool, desc, b.sampled_classes, 10, 2, 4)
    assert ops.is_point_major_view(b.x_all) == (layout == "pm") and b.x_all.shape == (3, 12, 9, N)
    x = torch.from_numpy(want["x"]).view(3, 12, 9, N)
    assert torch.equal(b.x_all.cpu(), x)
    assert torch.equal(b.support_x.cpu(), x[:, :10].reshape(3, 2, 5, 9, N)) and torch.equal(b.query_x.cpu(), x[:, 10:])
    assert torch.equal(b.support_flag.cpu(), torch.from_numpy(np.stack([p.support_flag for p in b.plans])))
    assert torch.equal(b.support_y.cpu(), torch.from_numpy(want["mask"]).view(3, 2, 5, N)) and b.support_y.dtype == torch.int32
    assert torch.equal(b.gt_support_y.cpu(), torch.from_numpy(want["gt_mask"]).view(3, 2, 5, N))
    assert torch.equal(b.query_y.cpu(), torch.from_numpy(want["query_y"]).view(3, 2, N))
    assert torch.equal(b.gt_query_y.cpu(), torch.from_numpy(want["gt_query_y"]).view(3, 2, N))
    assert torch.equal(b.slot_map.cpu(), torch.from_numpy(want["slot_map"]).view(3, 12, N))
    assert b.partial_info.dtype == torch.int32 and b.partial_info.shape == (3, 12, 8)
    assert torch.equal(b.partial_info.cpu(), torch.from_numpy(want["info"]).view(3, 12, 8))
    info = b.partial_info.cpu().view(36, 8).numpy()
    assert (info[noisy, 3] & 1).any() and np.all(info[~noisy] == 0) and np.all(info[noisy, 0] >= 3)   # a flip; no record elsewhere
    sup = np.nonzero(noisy.reshape(3, 12)[:, :10].reshape(30))[0]
    gt = b.gt_support_y.cpu().view(30, N)
    assert (gt[sup] == 0).all() and (gt.sum(1) > 0).sum() == 30 - len(sup)   # zero on the noisy shots, and only there
    assert b.support_y.sum(-1).min() > 0
    flipped = sup[(info[noisy, 3] & 1) != 0][0]                                # the flipped object's points are in the mask
    inst = pool.instances.cpu()[b.slot_map.cpu().view(36, N)[(flipped // 10) * 12 + flipped % 10].long()]
    row = info[(flipped // 10) * 12 + flipped % 10]
    assert (b.support_y.cpu().view(30, N)[flipped][inst == int(row[4])] == 1).all() and (inst == int(row[4])).sum() == row[5]


class _Hand:
    def __init__(self, blocks, class2scans):
        self.blocks, self.class2scans = blocks, class2scans

    def load(self, name):
        return self.blocks[name]


def _rows(labels, inst, seed):
    n = len(labels)
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 8))
    out[:, :3] = rs.uniform(-1, 2, (n, 3))
    out[:, 3:6] = rs.randint(0, 256, (n, 3))
    out[:, 6] = labels
    out[:, 7] = inst
    return out


C = 5  # the class of the hand-made clouds


def _hand_blocks():
    rs = np.random.RandomState(0)
    lab3 = lambda n: rs.choice([C, 7, 0], n)
    b = {}
    b["own"] = _rows(lab3(900), rs.permutation(900) - 450, 1)                       # every point its own object
    b["short"] = _rows(lab3(300), rs.randint(0, 6, 300), 2)                         # n < N: B', repeated slots
    ids = rs.choice([I32.min, -1, 0, I32.max], 700)                                 # the ends of int32 together
    b["edge"] = _rows(np.where(ids == 0, C, np.where(ids == -1, 0, 7)), ids, 3)     # object 0 is the class's: 3 eligible
    b["one_object"] = _rows(lab3(700), np.full(700, 3), 4)
    b["one_class"] = _rows(np.full(700, C), rs.randint(0, 6, 700), 5)
    # object 8: its first 80 points have label C, its other 120 label 7 -> the lowest slot decides: not eligible
    lab = np.concatenate([np.full(80, C), rs.choice([7, 0], 420), np.full(120, 7), np.full(80, C)])
    inst = np.concatenate([np.full(80, 8), rs.randint(1, 4, 420), np.full(120, 8), np.full(80, 9)])
    b["inconsistent"] = _rows(lab, inst, 6)
    b["alone"] = _rows(np.full(600, C), np.full(600, 4), 7)                         # one object of class C: a drop would empty it
    b["background"] = _rows(np.zeros(600), rs.randint(0, 5, 600), 8)                # no point of class C, one label: no flip
    b["big"] = _rows(lab3(16384), rs.randint(-20, 20, 16384), 9)                    # N = 8192: the LDS ceiling
    return b


@pytest.fixture(scope="module")
def hand():
    blocks = _hand_blocks()
    return BlockPool.from_source(_Hand(blocks, {C: list(blocks)}), instances=True)


def _one(hand, name, key, flags=6, n=N, seed=9):
    """One support cloud of block `name`: kernel against restatement, bit for bit -> the restatement's record."""
    desc = np.array([[hand.index[name], C, 0, flags, key]], np.int32)
    got, err = _raw(hand, desc, [[C]], 1, 0, seed, n=n, fill=-7)
    assert err is None, err
    want = _ref(hand, desc, np.array([[C]]), 1, 0, seed, n=n)
    _equal(got, want, what=name)
    return want["info"][0], want


@pytest.mark.parametrize("n", [512, 500])
def test_every_point_its_own_object(hand, n):
    info, _ = _one(hand, "own", 3, n=n)
    assert info[0] == n and info[1] > 0 and info[3] & 1 and info[5] == 1   # K == N: as many objects as slots


@pytest.mark.parametrize("name,flags", [("short", 6), ("edge", 6), ("one_object", 4), ("one_class", 6), ("inconsistent", 4)])
def test_hand_made_clouds(hand, name, flags):
    seen = set()
    for key in (0, 1, 2, 3):
        info, want = _one(hand, name, key, flags=flags)
        seen.add(int(info[4]))
        if name == "short":
            assert len(np.unique(want["slot_map"])) < N and info[3] & 1
        elif name == "edge":
            assert info[0] == 4 and info[1] == 3 and info[3] & 1 and info[4] in (I32.min, -1, I32.max)
        elif name == "one_object":
            assert info[0] == 1 and not info[3] & 1
        elif name == "one_class":
            assert info[0] == 6 and info[1] == 0 and not info[3] & 1
        else:
            sl = want["slot_map"][0] - int(hand.offsets[hand.index[name]])
            lab, inst = hand.labels.cpu().numpy(), hand.instances.cpu().numpy()
            o0 = int(hand.offsets[hand.index[name]])
            l8 = lab[o0 + sl][inst[o0 + sl] == 8]
            assert l8[0] == C and (l8 != C).any() and info[3] & 1 and info[4] in (1, 2, 3)   # 8 is never the flipped one
            assert np.array_equal(want["gt_mask"][0], (lab[o0 + sl] == C).astype(np.int32))       # flags 4: gt is mask0
    if name == "edge":
        assert len(seen) > 1


def _search(hand, name, seed, wanted):
    """The first key whose restated record has did & 6 == wanted."""
    o0, o1 = int(hand.offsets[hand.index[name]]), int(hand.offsets[hand.index[name] + 1])
    lab, inst = hand.labels.cpu().numpy()[o0:o1], hand.instances.cpu().numpy()[o0:o1]
    for key in range(200):
        sl = R.slots(lab, N, C, 0, seed, key)
        if P.edit(lab[sl], inst[sl], C, seed, key)[2][3] & 6 == wanted:
            return key
    raise AssertionError("no such key")


def test_a_drop_applied_and_a_drop_skipped(hand):
    key = _search(hand, "inconsistent", 9, 2)
    info, want = _one(hand, "inconsistent", key)
    assert info[3] & 2 and info[7] > 0 and want["mask"].sum() > 0
    key = _search(hand, "alone", 9, 4)
    info, want = _one(hand, "alone", key)
    assert info[3] == 4 and info[6] == 0 and info[7] == 0 and want["mask"].all()   # it would have emptied the mask
    key = _search(hand, "alone", 9, 0)
    info, want = _one(hand, "alone", key)
    assert info[3] == 0 and want["mask"].all()


def test_the_lds_ceiling(hand):
    info, want = _one(hand, "big", 5, n=8192)
    assert info[0] == 40 and info[3] & 1 and want["mask"].shape == (1, 8192)


def test_plain_descriptors_get_the_bits_of_the_plain_cut(pool):
    s = DeviceEpisodeSampler(pool, CLASSES, mode="test", noise_type="sym", noise_ratio=0.4, seed=8, **SHAPE)
    plans = [s.plan(), s.plan()]
    desc, classes = _keyed(plans, 0), np.stack([p.sampled_classes for p in plans])
    for layout in ("cm", "pm"):
        plain, e0 = _raw(pool, desc, classes, 10, 2, 8, fill=-7, partial=False, layout=layout)
        new, e1 = _raw(pool, desc, classes, 10, 2, 8, fill=-7, layout=layout)
        assert e0 is None and e1 is None
        for k in KEYS[:-1]:
            assert torch.equal(plain[k], new[k]), k
        assert (new["info"] == 0).all()
        got, err = _raw(pool, desc, classes, 10, 2, 8, fill=-7, instances=False, layout=layout)   # instance ids are not needed
        assert err is None and all(torch.equal(plain[k], got[k]) for k in KEYS[:-1])
    _equal(new, R.cut_batch(*[a for i, a in enumerate(_host(pool)) if i != 2], desc, classes, 10, 2, N, 8))


def test_bad_partial_descriptors_raise_and_touch_nothing_else(pool):
    s = DeviceEpisodeSampler(pool, CLASSES, mode="test", noise_type="sym", noise_ratio=0.4, seed=8, **SHAPE)
    plans = [s.plan(), s.plan()]
    good, classes = _keyed(plans, 0), np.stack([p.sampled_classes for p in plans])
    want = _ref(pool, good, classes, 10, 2, 8)
    plain_bit2, err = _raw(pool, np.where(np.arange(5) == 3, good | 4, good), classes, 10, 2, 8, fill=-7, partial=False)
    assert err is not None and "24 of 24 descriptors" in str(err)              # r3d_episode_cut still refuses bit 2
    cases = {"bit 2 on a query": (11, [(3, 5)], True), "bit 2 with m_A = 3": (4, [(3, 4), (2, 3)], True),
             "bit 2 without instance ids": (13, [(3, 4), (2, 0)], False)}
    for what, (row, edits, instances) in cases.items():
        desc = good.copy()
        for col, val in edits:
            desc[row, col] = val
        got, err = _raw(pool, desc, classes, 10, 2, 8, fill=-7, instances=instances)
        assert err is not None and "1 of 24 descriptors" in str(err) and "cloud %d" % row in str(err), (what, err)
        e, pos = divmod(row, 12)
        keep = torch.ones(24, dtype=torch.bool)
        keep[row] = False
        ks, kq = torch.ones(20, dtype=torch.bool), torch.ones(4, dtype=torch.bool)
        if pos < 10:
            ks[e * 10 + pos] = False
        else:
            kq[e * 2 + pos - 10] = False
        for k, sel in (("x", keep), ("slot_map", keep), ("info", keep), ("mask", ks), ("gt_mask", ks), ("query_y", kq),
                       ("gt_query_y", kq)):
            g = got[k].cpu()
            assert torch.equal(g[sel], torch.from_numpy(want[k])[sel]), (what, k)
            assert (g[~sel] == -7).all(), (what, k)                            # the refused cloud wrote nothing
    p = DeviceEpisodeSampler(pool, CLASSES, seed=8, **SHAPE, **PARTIAL)
    plans = [p.plan()]
    plans[0].desc[0, 2], plans[0].desc[0, 3] = 3, 6
    with pytest.raises(ValueError, match="cloud 0: flags 6"):                  # the sampler's own check speaks before any launch
        p.cut(plans, 0)


def test_an_empty_mask_raises_after_the_launch_and_the_cloud_is_written(hand):
    desc = np.array([[hand.index["inconsistent"], C, 0, 6, 1], [hand.index["background"], C, 0, 6, 2]], np.int32)
    got, err = _raw(hand, desc, [[C]], 2, 0, 9, fill=-7)
    assert err is not None and "1 of 2 clouds" in str(err) and "cloud 1" in str(err) and "without any point" in str(err)
    want = _ref(hand, desc, np.array([[C]]), 2, 0, 9)
    _equal(got, want)
    assert want["mask"][1].sum() == 0 and want["info"][1, 3] == 0 and want["info"][1, 1] == want["info"][1, 0] > 1
    assert (got["slot_map"].cpu()[1] >= int(hand.offsets[hand.index["background"]])).all()


def test_a_partial_batch_equals_single_cuts_and_repeats(pool):
    s = DeviceEpisodeSampler(pool, CLASSES, seed=6, **SHAPE, **PARTIAL)
    plans = [s.plan() for _ in range(3)]
    b = s.cut(plans, 7)
    assert s.counter == 0
    again = s.cut(plans, 7)
    names = ("x_all", "support_y", "gt_support_y", "query_y", "gt_query_y", "slot_map", "support_flag", "partial_info")
    for k in names + ("support_x", "query_x"):
        assert torch.equal(getattr(b, k), getattr(again, k)), k
    for e, p in enumerate(plans):
        one = s.cut([p], 7 + e)
        for k in names:
            assert torch.equal(getattr(one, k)[0], getattr(b, k)[e]), (e, k)
    other = s.cut(plans, 8)
    assert not torch.equal(other.partial_info, b.partial_info) or not torch.equal(other.slot_map, b.slot_map)


def test_evaluation_on_a_partial_batch(pool):
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    cfg = S.make_cfg(n_way=2, k_shot=5, n_queries=1, pc_npts=N, pretrain_checkpoint_path=None, model_checkpoint_path="synthetic")
    s = DeviceEpisodeSampler(pool, CLASSES, seed=1, **SHAPE, **PARTIAL)
    b = s.batch(2)
    assert (b.partial_info[..., 3] & 1).any()
    for L in (MPTILearner_V3(SimpleNamespace(**cfg), mode="test"), ProtoContrastLearner(SimpleNamespace(**cfg), mode="test")):
        out = L.test_batch([b.episode(e) for e in range(2)], None)
        assert len(out) == 2
        for pred, loss, acc in out:
            assert pred.shape == (2, N) and np.isfinite(float(loss)) and 0.0 <= acc <= 1.0
            assert int(pred.min()) >= 0 and int(pred.max()) <= 2
