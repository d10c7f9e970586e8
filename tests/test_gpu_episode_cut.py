"""r3d_episode_cut against its numpy restatement (tests/episode_cut_ref.py), bit for bit, and the DeviceEpisodeSampler
on top of it ("Cutting episodes on the device").  Blocks of 200 to 1200 points, N = 512, 2-way 2-shot,
one query per way: blocks on both sides of N, several 256-point rounds per pass, clouds in more than one workgroup."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import episode_cut_ref as R
from scene_ref import RefPlan
from r3dfsseg_amd import ops, synthetic as S
from r3dfsseg_amd.block_pool import ATTRIB_SETS, BlockPool, DeviceEpisodeSampler, share
from r3dfsseg_amd.episode_sampler import SyntheticBlocks

pytestmark = pytest.mark.gpu

CLASSES = list(range(1, 7))
N = 512
SHAPE = dict(n_way=2, k_shot=2, n_queries=1, num_point=N)


@pytest.fixture(scope="module")
def pool():
    return BlockPool.from_source(SyntheticBlocks(classes=CLASSES, scans_per_class=8, points_per_block=700, seed=1))


def _host(pool):
    return pool.points.cpu().numpy(), pool.labels.cpu().numpy(), pool.offsets.cpu().numpy()


def _ref(pool, desc, classes, Sn, Q, seed, attribs):
    return R.cut_batch(*_host(pool), desc, classes, Sn, Q, N, seed, attribs)


def _keyed(plans, counter):
    return np.concatenate([p.keyed(counter + e) for e, p in enumerate(plans)])


def _raw_cut(pool, desc, classes, Sn, Q, seed, attribs="xyzrgbXYZ", layout="cm", fill=None):
    """ops.episode_cut on tensors of the test's own (fill: what they hold before the launch) -> dict of tensors, error."""
    dev = pool.device
    C, rgb_ch, XYZ_ch = ATTRIB_SETS[attribs]
    E = classes.shape[0]
    B = E * (Sn + Q)
    mk = (lambda *s, dt: torch.empty(*s, device=dev, dtype=dt)) if fill is None else \
        (lambda *s, dt: torch.full(s, fill, device=dev, dtype=dt))
    x = mk(B, N, C, dt=torch.float32).transpose(1, 2) if layout == "pm" else mk(B, C, N, dt=torch.float32)
    out = dict(x=x, mask=mk(E * Sn, N, dt=torch.int32), gt_mask=mk(E * Sn, N, dt=torch.int32),
               query_y=mk(E * Q, N, dt=torch.int64), gt_query_y=mk(E * Q, N, dt=torch.int64), slot_map=mk(B, N, dt=torch.int32))
    err = None
    try:
        ops.episode_cut(pool.points, pool.labels, pool.offsets, torch.from_numpy(np.ascontiguousarray(desc, np.int32)).to(dev),
                        torch.from_numpy(np.ascontiguousarray(classes, np.int32)).to(dev), Sn, Q, N, seed, x, rgb_ch, XYZ_ch,
                        out["mask"], out["gt_mask"], out["query_y"], out["gt_query_y"], out["slot_map"])
    except ValueError as e:
        err = e
    return out, err


def _equal(got, want, rows=None, what=""):
    for k, w in want.items():
        g = got[k].cpu()
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape)
        assert torch.equal(g, w), (what, k)


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("attribs", ["xyz", "xyzrgbXYZ"])
def test_batch_equals_the_restatement_bit_for_bit(pool, layout, attribs):
    s = DeviceEpisodeSampler(pool, CLASSES, mode="train", noise_ratio=[0.0, 0.5], seed=4, pc_attribs=attribs, layout=layout, **SHAPE)
    b = s.batch(3)
    assert s.counter == 3 and b.E == 3 and b.sampled_classes.shape == (3, 2)
    desc = _keyed(b.plans, 0)
    sizes = np.array([pool.size(k) for k in desc[:, 0]])
    assert (sizes < N).any() and (sizes >= N).any()                # both B' and B
    assert (desc[:, 3] & 2).any() and not (desc[:, 3] & 2).all()   # noisy and clean shots
    want = _ref(pool, desc, b.sampled_classes, 4, 2, 4, attribs)
    C = ATTRIB_SETS[attribs][0]
    assert b.x_all.shape == (3, 6, C, N) and ops.is_point_major_view(b.x_all) == (layout == "pm")
    assert ops.is_point_major_view(b.support_x) == (layout == "pm") and b.support_x.shape == (3, 2, 2, C, N)
    x = torch.from_numpy(want["x"]).view(3, 6, C, N)
    assert torch.equal(b.x_all.cpu(), x)
    assert torch.equal(b.support_x.cpu(), x[:, :4].reshape(3, 2, 2, C, N)) and torch.equal(b.query_x.cpu(), x[:, 4:])
    assert torch.equal(b.support_y.cpu(), torch.from_numpy(want["mask"]).view(3, 2, 2, N)) and b.support_y.dtype == torch.int32
    assert torch.equal(b.gt_support_y.cpu(), torch.from_numpy(want["gt_mask"]).view(3, 2, 2, N))
    assert torch.equal(b.query_y.cpu(), torch.from_numpy(want["query_y"]).view(3, 2, N)) and b.query_y.dtype == torch.int64
    assert torch.equal(b.gt_query_y.cpu(), torch.from_numpy(want["gt_query_y"]).view(3, 2, N))
    assert torch.equal(b.slot_map.cpu(), torch.from_numpy(want["slot_map"]).view(3, 6, N))
    assert torch.equal(b.support_flag.cpu(), torch.from_numpy(np.stack([p.support_flag for p in b.plans])))
    assert b.support_y.sum(-1).min() > 0 and (b.gt_support_y.sum(-1) == 0).any() and b.query_y.max() <= 2


class _Hand:
    def __init__(self, blocks, class2scans):
        self.blocks, self.class2scans = blocks, class2scans

    def load(self, name):
        return self.blocks[name]


def _rows(n, labels, seed):
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 7))
    out[:, :3] = rs.uniform(-1, 2, (n, 3))
    out[:, 3:6] = rs.randint(0, 256, (n, 3))
    out[:, 6] = labels
    return out


def test_boundary_blocks():
    """n == N, n == N - 1, one point, a block that is all one class (m_A == N, m_B == 0), a block flat in z; each cut as a
    support cloud and as a query cloud."""
    half = lambda n: (np.arange(n) % 3 == 0) * 1 + (np.arange(n) % 3 == 1) * 2
    flat = _rows(700, half(700), 5)
    flat[:, 2] = 1.25
    blocks = {"exact": _rows(N, half(N), 1), "short": _rows(N - 1, half(N - 1), 2), "one": _rows(1, [1], 3),
              "full": _rows(600, np.ones(600), 4), "flat": flat}
    pool = BlockPool.from_source(_Hand(blocks, {1: list(blocks), 2: ["exact", "short", "flat"]}))
    names = list(blocks)
    m = [share(pool.count(k, 1), pool.size(k), N) for k in names]
    assert m[names.index("full")] == N and m[names.index("one")] == 1 and m[names.index("short")] == pool.count("short", 1)
    desc = np.array([[pool.index[k], 1, m[i], 0, 100 + i] for i, k in enumerate(names)] +
                    [[pool.index[k], 1, m[i], 1, 200 + i] for i, k in enumerate(names)], np.int32)
    classes = np.array([[2, 1]], np.int32)
    for attribs in ("xyzrgbXYZ", "xyz"):
        got, err = _raw_cut(pool, desc, classes, 5, 5, seed=9, attribs=attribs)
        assert err is None
        want = _ref(pool, desc, classes, 5, 5, 9, attribs)
        _equal(got, want, what=attribs)
    x = got["x"]  # (10, 3, N) of the last round; the 9-channel one is in `want` of the first: check the flat axis there
    want9 = _ref(pool, desc, classes, 5, 5, 9, "xyzrgbXYZ")["x"]
    assert np.all(want9[names.index("flat"), 8] == 0) and np.all(want9[names.index("flat"), 2] == 0)   # z - min, Z: 0, no NaN
    assert np.all(want9[names.index("one"), 6:9] == 0) and np.isfinite(want9).all()
    assert np.all(got["mask"].cpu().numpy()[names.index("full")] == 1) and np.all(got["query_y"].cpu().numpy()[names.index("full")] == 2)


def test_a_batch_equals_single_cuts_and_repeats(pool):
    s = DeviceEpisodeSampler(pool, CLASSES, mode="train", noise_ratio=[0.0, 0.5], seed=6, **SHAPE)
    plans = [s.plan() for _ in range(3)]
    b = s.cut(plans, 7)
    assert s.counter == 0  # an explicit counter leaves the sampler's own alone
    again = s.cut(plans, 7)
    for k in ("x_all", "support_x", "query_x", "support_y", "gt_support_y", "query_y", "gt_query_y", "slot_map", "support_flag"):
        assert torch.equal(getattr(b, k), getattr(again, k)), k
    for e, p in enumerate(plans):
        one = s.cut([p], 7 + e)
        for k in ("x_all", "support_y", "gt_support_y", "query_y", "gt_query_y", "slot_map", "support_flag"):
            assert torch.equal(getattr(one, k)[0], getattr(b, k)[e]), (e, k)
    other = s.cut(plans, 8)
    assert not torch.equal(other.slot_map, b.slot_map)  # the key decides the draw


def test_same_arithmetic_as_scene_prepare(pool):
    """The pool rows of a cloud's slot_map, prepared by the restatement of r3d_scene_prepare (tests/scene_ref.py, step 6)."""
    s = DeviceEpisodeSampler(pool, CLASSES, mode="test", noise_type="sym", noise_ratio=0.5, seed=2, **SHAPE)
    b = s.batch(2)
    ref = object.__new__(RefPlan)  # step 6 alone: it reads the scan, the slot map and N
    ref.scan, ref.N = pool.points.cpu().numpy(), N
    ref.slot_map = b.slot_map.cpu().numpy().reshape(-1, N)
    assert torch.equal(b.x_all.cpu().reshape(-1, 9, N), torch.from_numpy(ref.prepared(rgb=True, XYZ=True)))


def test_augmentation_on_top(pool):
    from r3dfsseg_amd.augment import augment_clouds
    s = DeviceEpisodeSampler(pool, CLASSES, mode="train", noise_ratio=[0.5], seed=3, **SHAPE)
    b = s.batch(2)
    cfg = {"scale": 1.1, "rot": 1, "mirror_prob": 0.5, "jitter": 1}
    a = b.augmented(cfg, seed=5, counter=3)
    want = augment_clouds(b.x_all.reshape(12, 9, N), cfg, 5, 3 * 6).reshape(2, 6, 9, N)
    assert torch.equal(a.x_all, want) and not torch.equal(a.x_all, b.x_all)
    assert a.support_y is b.support_y and torch.equal(a.support_x.reshape(2, 4, 9, N), want[:, :4])


def test_training_on_a_cut_batch(pool):
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    cfg = S.make_cfg(n_way=2, k_shot=2, pc_npts=N, pretrain_checkpoint_path="synthetic", model_checkpoint_path=None, lr=1e-3,
                     step_size=5000, gamma=0.5)
    L = MPTILearner_V3(SimpleNamespace(**cfg), mode="train")
    L.model.att_learner.dropout.p = 0.0
    L.model._lp_budget = 150
    s = DeviceEpisodeSampler(pool, CLASSES, mode="train", noise_ratio=[0.0, 0.5], seed=1, **SHAPE)
    b = s.batch(2)
    before = torch.cat([p.detach().reshape(-1) for p in L.model.parameters()]).clone()
    out = L.train_batch([b.episode(e) for e in range(2)], None)
    assert len(out) == 2 and all(len(o) == 8 for o in out)
    assert all(np.isfinite(float(o[0])) and np.isfinite(float(o[1])) and np.isfinite(float(o[2])) for o in out)
    after = torch.cat([p.detach().reshape(-1) for p in L.model.parameters()])
    assert torch.isfinite(after).all() and (after - before).abs().max().item() > 0


def test_bad_descriptors_raise_and_touch_nothing_else(pool):
    """An error return, not a fault: the kernel bounds every index it takes from a descriptor before using it.  The refused
    cloud keeps what its tensors held; its neighbours are what the restatement says."""
    s = DeviceEpisodeSampler(pool, CLASSES, mode="test", noise_type="sym", noise_ratio=0.5, seed=8, **SHAPE)
    plans = [s.plan(), s.plan()]
    good = _keyed(plans, 0)
    classes = np.stack([p.sampled_classes for p in plans])
    want = _ref(pool, good, classes, 4, 2, 8, "xyzrgbXYZ")
    cases = {"block past the pool": (1, 0, len(pool) + 5), "negative block": (4, 0, -1),
             "m_A above the class's points": (7, 2, pool.count(good[7, 0], good[7, 1]) + 1), "m_A above N": (2, 2, N + 1),
             "negative m_A": (10, 2, -3), "a query flag on a support cloud": (3, 3, 1)}
    for what, (row, col, val) in cases.items():
        desc = good.copy()
        desc[row, col] = val
        got, err = _raw_cut(pool, desc, classes, 4, 2, seed=8, fill=-7)
        assert err is not None and "1 of 12 descriptors" in str(err) and "cloud %d" % row in str(err), (what, err)
        e, pos = divmod(row, 6)
        keep = torch.ones(12, dtype=torch.bool)
        keep[row] = False
        ks = torch.ones(8, dtype=torch.bool)
        kq = torch.ones(4, dtype=torch.bool)
        if pos < 4:
            ks[e * 4 + pos] = False
        else:
            kq[e * 2 + pos - 4] = False
        for k, sel in (("x", keep), ("slot_map", keep), ("mask", ks), ("gt_mask", ks), ("query_y", kq), ("gt_query_y", kq)):
            g = got[k].cpu()
            assert torch.equal(g[sel], torch.from_numpy(want[k])[sel]), (what, k)
            assert (g[~sel] == -7).all(), (what, k)  # the refused cloud wrote nothing
    with pytest.raises(ValueError, match="cloud 1: block"):  # the sampler's own check speaks before any launch
        plans[0].desc[1, 0] = len(pool) + 5
        s.cut(plans, 0)
