"""--pc_augm on the device (csrc/augment.hip, r3dfsseg_amd/augment.py): the kernel against the reference's own outputs
(tests/golden/augment.npz, dataloaders/loader.py:205-213,354-373) and against float64 numpy, what it draws, its keys, and the
learners' switch.

Bars.  xyz' is a three-term fp32 dot of |x| <= 4 with |M| <= 1.2 plus the noise: each product and sum rounds at <= 2^-24 of
<= 5, and M and the noise are rounded to fp32 on the way in; together about 3e-6, asserted at 1e-5.  XYZ' divides a
difference of two such values by the extent, so its bar is 3e-5 / min_extent with min_extent the smallest extent of any
augmented cloud (stored in the fixture; computed from the float64 reference for the other shapes)."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")
FULL = {"scale": 1.2, "rot": 1, "mirror_prob": 1.0, "jitter": 1}
OFF = {"scale": 0, "rot": 0, "mirror_prob": 0, "jitter": 0}
XYZ_TOL, XYZN_TOL = 1e-5, 3e-5


def _cfg(v):
    return {"scale": float(v[0]), "rot": int(v[1]), "mirror_prob": float(v[2]), "jitter": int(v[3])}


def _clouds(xyz, C, seed=0):
    """xyz (B, N, 3) float32 -> point-major (B, N, C) float32: xyz | rgb | XYZ of the input (as a prepared cloud holds)."""
    B, N, _ = xyz.shape
    parts = [xyz]
    if C >= 6:
        parts.append(np.random.RandomState(seed).rand(B, N, 3).astype(np.float32))
    if C == 9:
        d = xyz - xyz.min(axis=1, keepdims=True)
        parts.append(d / d.max(axis=1, keepdims=True))
    return np.ascontiguousarray(np.concatenate(parts, axis=2).astype(np.float32))


def _dev(pm, layout):
    """(B, N, C) numpy -> (B, C, N) device tensor: contiguous channel-major ('cm') or a point-major view ('pm')."""
    t = torch.from_numpy(pm).cuda()
    return t.transpose(1, 2).contiguous() if layout == "cm" else t.transpose(1, 2)


def _host(t):
    """(B, C, N) device tensor -> (B, N, C) numpy."""
    return t.detach().cpu().transpose(1, 2).contiguous().numpy()


def _reference(xyz, mats, noise):
    """float64: xyz' = xyz . M^T + noise and XYZ' (loader.py:368-372, 210-213) from the fp32 values the kernel is given."""
    out = np.einsum("bnj,bij->bni", xyz.astype(np.float64), mats.astype(np.float64).reshape(-1, 3, 3))
    if noise is not None:
        out = out + noise.astype(np.float64)
    d = out - out.min(axis=1, keepdims=True)
    return out, d / d.max(axis=1, keepdims=True), float(d.max(axis=1).min())


def _check(got, pm_in, want_xyz, want_XYZ, min_extent, C):
    e_xyz = np.abs(got[:, :, 0:3].astype(np.float64) - want_xyz).max()
    print("xyz err %.3g (bar %.3g)" % (e_xyz, XYZ_TOL))
    assert e_xyz <= XYZ_TOL
    if C >= 6:
        assert np.array_equal(got[:, :, 3:6].view(np.uint32), pm_in[:, :, 3:6].view(np.uint32))
    if C == 9:
        e_n = np.abs(got[:, :, 6:9].astype(np.float64) - want_XYZ).max()
        print("XYZ err %.3g (bar %.3g)" % (e_n, XYZN_TOL / min_extent))
        assert e_n <= XYZN_TOL / min_extent


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("config", [0, 1])
def test_parity_with_the_reference(config, layout):
    """The reference's M and noise in, the reference's xyz' and XYZ' out; N = 250 leaves a tail in the 256-thread group."""
    from r3dfsseg_amd.augment import augment_clouds
    g = np.load(GOLDEN)
    pre = "c%d/" % config
    pm = _clouds(g["x"].astype(np.float32), 9)
    x = _dev(pm, layout)
    out = augment_clouds(x, _cfg(g[pre + "cfg"]), seed=1, mats=g[pre + "M"].reshape(-1, 9), noise=g[pre + "noise"])
    assert out.shape == x.shape and out.stride() == x.stride()
    assert np.array_equal(_host(x), pm)  # the input is left alone
    _check(_host(out), pm, g[pre + "xyz"], g[pre + "XYZ"], float(g["min_extent"]), 9)


@pytest.mark.parametrize("layout", ["cm", "pm"])
@pytest.mark.parametrize("C,N", [(3, 37), (6, 37), (9, 37), (3, 600), (6, 600), (9, 600)])
def test_other_shapes_against_float64(C, N, layout):
    """No XYZ (C = 3, 6), fewer points than threads (37), several points per thread and no multiple of 256 (600)."""
    from r3dfsseg_amd import episode_sampler as ES
    from r3dfsseg_amd.augment import augment_clouds
    import random
    B = 3
    rs = np.random.RandomState(100 + N)
    xyz = (rs.rand(B, N, 3) * [1.0, 1.0, 3.0]).astype(np.float32)
    xyz = xyz - xyz.min(axis=1, keepdims=True)
    pyrng = random.Random(N)
    mats = np.stack([ES.augment_matrix(FULL, pyrng) for _ in range(B)]).astype(np.float32).reshape(B, 9)
    noise = np.clip(0.01 * rs.randn(B, N, 3), -0.05, 0.05).astype(np.float32)
    pm = _clouds(xyz, C, seed=N)
    want_xyz, want_XYZ, min_extent = _reference(xyz, mats, noise)
    assert min_extent >= 0.5
    got = _host(augment_clouds(_dev(pm, layout), FULL, seed=1, mats=mats, noise=noise))
    _check(got, pm, want_xyz, want_XYZ, min_extent, C)


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_identity(layout):
    """Nothing switched on: xyz and rgb are the input's bits, XYZ the input's XYZ to 1e-6."""
    from r3dfsseg_amd.augment import augment_clouds
    pm = _clouds(np.load(GOLDEN)["x"].astype(np.float32), 9)
    out, mats = augment_clouds(_dev(pm, layout), OFF, seed=5, return_mats=True)
    got = _host(out)
    assert np.array_equal(mats.cpu().numpy(), np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (4, 1)))
    assert np.array_equal(got[:, :, 0:6].view(np.uint32), pm[:, :, 0:6].view(np.uint32))
    assert np.abs(got[:, :, 6:9] - pm[:, :, 6:9]).max() <= 1e-6


def _drawn(cfg, B=64, seed=3, first_key=0):
    from r3dfsseg_amd.augment import augment_clouds
    x = torch.rand(B, 3, 16, device="cuda")
    _, mats = augment_clouds(x, cfg, seed=seed, first_key=first_key, return_mats=True)
    return mats.cpu().numpy().astype(np.float64).reshape(B, 3, 3)


def test_drawn_matrices():
    M = _drawn(FULL)
    s = M[:, 2, 2]
    assert (s >= 1 / 1.2 - 1e-6).all() and (s <= 1.2 + 1e-6).all() and s.std() > 0.02
    assert np.abs(np.einsum("bki,bkj->bij", M, M) - (s ** 2)[:, None, None] * np.eye(3)).max() <= 1e-5
    assert (M[:, 2, 0] == 0).all() and (M[:, 2, 1] == 0).all() and (M[:, 0, 2] == 0).all() and (M[:, 1, 2] == 0).all()
    for scale in (0, 0.5, 1.0):  # s == 1 exactly when scale <= 1
        M = _drawn(dict(FULL, scale=scale))
        assert (M[:, 2, 2] == 1.0).all()
        assert np.abs(np.einsum("bki,bkj->bij", M, M) - np.eye(3)).max() <= 1e-5
    M = _drawn(dict(FULL, rot=0, mirror_prob=0))  # no rotation, no mirror: s I
    assert (M == M[:, 2, 2][:, None, None] * np.eye(3)).all() and M[:, 2, 2].std() > 0.02
    M = _drawn(dict(FULL, mirror_prob=0))  # a proper rotation
    assert (np.linalg.det(M) > 0).all()
    M = _drawn(dict(FULL, rot=0, mirror_prob=2))  # probability 2 / 2: both mirrors on every cloud
    s = M[:, 2, 2]
    assert (M == s[:, None, None] * np.diag([-1.0, -1.0, 1.0])).all()


def test_drawn_matrices_statistics():
    """4096 keys: each mirror fires with probability mirror_prob / 2 = 0.5 (a mirrored cloud with 0.75), within 5 binomial
    standard deviations; the angles reach all four quadrants, about a quarter of the clouds each."""
    n = 4096
    M = _drawn(dict(OFF, mirror_prob=1.0), B=n, seed=9)
    mx, my = M[:, 0, 0] < 0, M[:, 1, 1] < 0
    for frac, p in ((mx.mean(), 0.5), (my.mean(), 0.5), ((mx | my).mean(), 0.75), ((mx & my).mean(), 0.25)):
        print("mirror fraction %.4f (expected %.2f)" % (frac, p))
        assert abs(frac - p) <= 5 * np.sqrt(p * (1 - p) / n)
    M = _drawn(dict(OFF, rot=1), B=n, seed=9)
    ang = np.arctan2(M[:, 1, 0], M[:, 0, 0])
    quad = np.floor((ang % (2 * np.pi)) / (np.pi / 2)).astype(int).clip(0, 3)
    counts = np.bincount(quad, minlength=4)
    print("quadrants", counts.tolist())
    assert (np.abs(counts / n - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / n)).all()
    assert np.abs(M[:, 0, 0] - M[:, 1, 1]).max() == 0 and np.abs(M[:, 0, 1] + M[:, 1, 0]).max() == 0


def test_drawn_jitter():
    from r3dfsseg_amd.augment import augment_clouds
    B, N = 4, 512
    rs = np.random.RandomState(2)
    xyz = (rs.rand(B, N, 3) * [1.0, 1.0, 3.0]).astype(np.float32)
    pm = _clouds(xyz, 9)
    got = _host(augment_clouds(_dev(pm, "cm"), dict(OFF, jitter=1), seed=21))
    d = got[:, :, 0:3].astype(np.float64) - xyz.astype(np.float64)
    print("jitter: max %.4f mean %.3g std %.5f" % (np.abs(d).max(), d.mean(), d.std()))
    assert np.abs(d).max() <= 0.05 + 1e-6
    assert abs(d.mean()) <= 5 * 0.01 / np.sqrt(d.size) and d.size == 6144
    assert abs(d.std() - 0.01) <= 0.05 * 0.01
    assert np.array_equal(got[:, :, 3:6], pm[:, :, 3:6])
    for a in range(B):  # clouds with different keys differ
        for b in range(a + 1, B):
            assert np.abs(d[a] - d[b]).max() > 0.01
    for i, j in ((0, 1), (0, 2), (1, 2)):  # the three axes of a point differ
        assert (np.abs(d[:, :, i] - d[:, :, j]) > 1e-6).mean() > 0.99


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_XYZ_is_consistent_with_the_xyz_written(layout):
    from r3dfsseg_amd.augment import augment_clouds
    rs = np.random.RandomState(4)
    pm = _clouds((rs.rand(3, 600, 3) * [1.0, 1.0, 3.0]).astype(np.float32), 9)
    got = _host(augment_clouds(_dev(pm, layout), FULL, seed=8))
    v = got[:, :, 0:3]
    d = v - v.min(axis=1, keepdims=True)  # float32 throughout
    want = d / d.max(axis=1, keepdims=True)
    assert want.dtype == np.float32 and np.abs(got[:, :, 6:9] - want).max() <= 1e-6
    assert (got[:, :, 6:9].min(axis=1) == 0.0).all() and (got[:, :, 6:9].max(axis=1) == 1.0).all()


@pytest.mark.parametrize("layout", ["cm", "pm"])
def test_determinism_seeds_and_in_place(layout):
    from r3dfsseg_amd.augment import augment_clouds
    rs = np.random.RandomState(6)
    pm = _clouds((rs.rand(5, 300, 3) * [1.0, 1.0, 3.0]).astype(np.float32), 9)
    x = _dev(pm, layout)
    a = augment_clouds(x, FULL, seed=40, first_key=7)
    assert torch.equal(a, augment_clouds(x, FULL, seed=40, first_key=7))
    b = augment_clouds(x, FULL, seed=41, first_key=7)
    assert not torch.equal(a[:, 0:3], b[:, 0:3])
    one = torch.ones(1, device="cuda", dtype=torch.int32)
    assert torch.equal(b, augment_clouds(x, FULL, seed=40, first_key=7, seed_dev=one))
    # cloud b of a call with first_key k is cloud 0 of a call with first_key k + b
    assert torch.equal(a[2:3], augment_clouds(x[2:3], FULL, seed=40, first_key=9))
    assert not torch.equal(a[2:3, 0:3], augment_clouds(x[2:3], FULL, seed=40, first_key=10)[:, 0:3])
    y = _dev(pm, layout)
    assert augment_clouds(y, FULL, seed=40, first_key=7, out=y) is y
    assert torch.equal(y, a) and y.stride() == a.stride()


def _episodes(n, pm=False, seed0=70):
    from r3dfsseg_amd import synthetic as S
    cfg = S.make_cfg(n_way=2, k_shot=2, pc_npts=512)
    eps = []
    for e in range(n):
        data, _ = S.make_episode(cfg, seed=seed0 + e, noise_ratio=0.5, train=True)
        data = [t.cuda() for t in data]
        if pm:
            for i in (0, 2):
                data[i] = data[i].transpose(-1, -2).contiguous().transpose(-1, -2)
        eps.append(data)
    return eps


@pytest.mark.parametrize("pm", [False, True])
def test_batch_equals_single_episodes(pm):
    """EpisodeBatch.augmented on E = 3 episodes at counter c == three augment_episode calls with c, c + 1, c + 2, bit for bit."""
    from r3dfsseg_amd import ops
    from r3dfsseg_amd.augment import augment_episode
    from r3dfsseg_amd.batch import EpisodeBatch
    eps = _episodes(3, pm)
    b0 = EpisodeBatch.from_episodes(eps)
    b = b0.augmented(FULL, 13, 5)
    assert b.x_all.shape == b0.x_all.shape and ops.is_point_major_view(b.x_all) == pm and b.support_y is b0.support_y
    assert ops.is_point_major_view(b.support_x) == pm and ops.is_point_major_view(b.query_x) == pm
    S = 4
    for e, ep in enumerate(eps):
        one = augment_episode(ep, FULL, 13, 5 + e)
        assert len(one) == len(ep) and all(one[i] is ep[i] for i in range(len(ep)) if i not in (0, 2))
        assert one[0].shape == ep[0].shape and not torch.equal(one[0], ep[0]) and ops.is_point_major_view(one[0]) == pm
        assert torch.equal(b.x_all[e, :S], one[0].reshape(S, 9, 512)) and torch.equal(b.x_all[e, S:], one[2])
        assert torch.equal(b.support_x[e], one[0]) and torch.equal(b.query_x[e], one[2])
    assert torch.equal(b0.x_all[0, :S], eps[0][0].reshape(S, 9, 512))  # the source batch is left alone


def _raw(x, out, B, C, N, xyz_ch=0, XYZ_ch=-1):
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    _lib.check(lib.r3d_augment_clouds(p(x), C * N, N, 1, p(out), C * N, N, 1, B, C, N, xyz_ch, XYZ_ch, 1.2, 1, 1.0, 1, 0, None, 0,
                                      None, None, None, None))


def test_bad_arguments_raise_with_the_library_message():
    buf = torch.zeros(2 * 9 * 16, device="cuda")
    for kw, word in ((dict(B=0, C=9, N=16), "B 0"), (dict(B=2, C=9, N=0), "N 0"), (dict(B=2, C=9, N=-3), "N -3"),
                     (dict(B=2, C=4, N=16), "C 4"), (dict(B=2, C=12, N=8), "C 12"),
                     (dict(B=2, C=3, N=16, xyz_ch=1), "xyz_ch 1"), (dict(B=2, C=9, N=16, xyz_ch=-1), "xyz_ch -1"),
                     (dict(B=2, C=9, N=16, XYZ_ch=7), "XYZ_ch 7"), (dict(B=2, C=9, N=16, XYZ_ch=-2), "XYZ_ch -2"),
                     (dict(B=2, C=9, N=16, XYZ_ch=2), "overlap")):
        with pytest.raises(RuntimeError, match="r3d_augment_clouds.*" + word):
            _raw(buf, buf, **kw)
    for x, out in ((None, buf), (buf, None)):
        with pytest.raises(RuntimeError, match="r3d_augment_clouds: null pointer"):
            _raw(x, out, B=2, C=9, N=16)
    from r3dfsseg_amd.augment import augment_clouds
    with pytest.raises(RuntimeError, match="r3d_augment_clouds: C 4"):
        augment_clouds(torch.zeros(2, 4, 16, device="cuda"), FULL, seed=0)
    with pytest.raises(KeyError):
        augment_clouds(torch.zeros(2, 3, 16, device="cuda"), {"scale": 1.2}, seed=0)


# ---------------------------------------------------------------------------------------------------------- learners
SEED = 11
AUGM = dict(pc_augm=True, pc_augm_scale=1.2, pc_augm_rot=1, pc_augm_mirror_prob=1.0, pc_augm_jitter=1)


def _learner_cfg(**over):
    from r3dfsseg_amd import synthetic as S
    return S.make_cfg(n_way=2, k_shot=2, pc_npts=512, pretrain_checkpoint_path="synthetic", model_checkpoint_path=None,
                      lr=1e-3, step_size=5000, gamma=0.5, **over)


def _mpti(**over):
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    L = MPTILearner_V3(SimpleNamespace(**_learner_cfg(**over)), mode="train")
    L.model.att_learner.dropout.p = 0.0
    L.model._lp_budget = 150
    return L


def _proto(**over):
    from r3dfsseg_amd.proto_learner import ProtoLearner
    L = ProtoLearner(SimpleNamespace(**_learner_cfg(**over)), mode="train")
    L.model.att_learner.dropout.p = 0.0
    return L


def _floats(t):
    return tuple(float(v.detach()) if torch.is_tensor(v) else float(v) for v in t)


def test_mpti_train_augments_on_the_device():
    """Learner A (device_augm + pc_augm) on raw episodes == learner B (no augmentation) on augment_episode(ep, cfg, seed, k):
    the same train() tuple bit for bit, call after call (A's counter advances per episode)."""
    from r3dfsseg_amd.augment import augment_episode, config_from_args
    eps = _episodes(2)
    A, B = _mpti(device_augm=True, device_augm_seed=SEED, **AUGM), _mpti()
    cfg = config_from_args(SimpleNamespace(**AUGM))
    assert cfg == FULL
    plain = _floats(_mpti().train(eps[0], None))
    for k, ep in enumerate(eps):
        got = _floats(A.train(ep, None))
        want = _floats(B.train(augment_episode(ep, cfg, SEED, k), None))
        assert len(got) == 8 and got == want
        if k == 0:
            assert got != plain  # and the augmentation is not a no-op
    for (k, va), (_, vb) in zip(A.model.state_dict().items(), B.model.state_dict().items()):
        assert torch.equal(va, vb), k


def test_mpti_train_batch_augments_on_the_device():
    from r3dfsseg_amd.augment import augment_episode
    eps = _episodes(4)
    A, B = _mpti(device_augm=True, device_augm_seed=SEED, **AUGM), _mpti()
    for step in range(2):  # the second step: counters 2, 3
        batch = eps[2 * step:2 * step + 2]
        got = [_floats(o) for o in A.train_batch(batch, None)]
        want = [_floats(o) for o in B.train_batch([augment_episode(ep, FULL, SEED, 2 * step + e) for e, ep in enumerate(batch)],
                                                  None)]
        assert len(got) == 2 and all(len(o) == 8 for o in got) and got == want
    assert torch.equal(A._batch_trainer.bucket.flat, B._batch_trainer.bucket.flat)


def test_proto_train_and_train_batch_augment_on_the_device():
    from r3dfsseg_amd.augment import augment_episode
    eps = _episodes(3)
    A, B = _proto(device_augm=True, device_augm_seed=SEED, **AUGM), _proto()
    got = _floats(A.train(eps[0], None))
    assert len(got) == 2 and got == _floats(B.train(augment_episode(eps[0], FULL, SEED, 0), None))
    got = [_floats(o) for o in A.train_batch(eps[1:3], None)]
    want = [_floats(o) for o in B.train_batch([augment_episode(ep, FULL, SEED, 1 + e) for e, ep in enumerate(eps[1:3])], None)]
    assert got == want and len(got) == 2 and A._augm.counter == 3


def test_switch_needs_both_flags_and_test_is_unaffected():
    """device_augm with pc_augm unset, and pc_augm alone (the reference's own flag: its dataset already augmented on the
    host), both train on the clouds as they come; test() never augments."""
    from r3dfsseg_amd import synthetic as S
    eps = _episodes(1)
    tdata, sc = S.make_episode(_learner_cfg(), seed=90, noise_ratio=0.5)
    tdata = [t.cuda() for t in tdata]
    ref = _mpti()
    pred0, loss0, acc0 = ref.test(tdata, sc)
    On = _mpti(device_augm=True, device_augm_seed=SEED, **AUGM)
    pred, loss, acc = On.test(tdata, sc)
    assert torch.equal(pred, pred0) and float(loss) == float(loss0) and acc == acc0 and On._augm.counter == 0
    want = _floats(ref.train(eps[0], None))
    assert _floats(_mpti(device_augm=True, device_augm_seed=SEED).train(eps[0], None)) == want
    assert _floats(_mpti(**AUGM).train(eps[0], None)) == want
    assert _floats(On.train(eps[0], None)) != want and On._augm.counter == 1
    P0, P1 = _proto(), _proto(device_augm=True, device_augm_seed=SEED, **AUGM)
    a, b = P0.test(tdata, sc), P1.test(tdata, sc)
    assert torch.equal(a[0], b[0]) and float(a[1]) == float(b[1]) and a[2] == b[2]
    assert _floats(_proto(device_augm=True).train(eps[0], None)) == _floats(P0.train(eps[0], None))
