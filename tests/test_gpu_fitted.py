"""A support set fitted once (r3dfsseg_amd/fitted.py): model.fit_support + model.predict on the device.

The bar is torch.equal everywhere: predict on a query group gives the bits of forward() on the episode [that support set |
that group].  That rests on what test_batch == test() already rests on: a cloud's features do not depend on how many clouds
share the encoder call.  No tolerance is used in this file."""
import ctypes
import gc
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r3dfsseg_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (model class, cfg overrides, noise_ratio, eval flag)
CASES = {
    "proto_cos": ("ProtoNet", dict(n_way=2, k_shot=1, pc_npts=512, dist_method="cosine"), 0.0, False),
    "proto_euc": ("ProtoNet", dict(n_way=2, k_shot=1, pc_npts=512, dist_method="euclidean"), 0.0, False),
    "contrast": ("ProtoNet_Contrast", dict(n_way=2, k_shot=5, pc_npts=512), 0.4, False),
    "mpti_fps": ("MPTI_SelfAtten", dict(n_way=2, k_shot=2, pc_npts=512, n_subprototypes=20), 0.0, False),
    "mpti_eval": ("MPTI_SelfAtten", dict(n_way=2, k_shot=5, pc_npts=512), 0.4, True),
    "mpti_4way": ("MPTI_SelfAtten", dict(n_way=4, k_shot=1, pc_npts=256), 0.0, False),
}
MPTI = [c for c in CASES if c.startswith("mpti")]
_cache = {}


def _model(name):
    """(model, cfg, episode on the device, eval flag) of a case, built once per session."""
    if name not in _cache:
        from r3dfsseg_amd import mpti, protonet
        cls_name, over, noise, ev = CASES[name]
        cfg = S.make_cfg(**over)
        cls = getattr(mpti, cls_name, None) or getattr(protonet, cls_name)
        m = cls(SimpleNamespace(**cfg))
        sd = S.make_state_dict(cfg, 123)
        m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()})
        m.cuda().eval()
        ep = [t.cuda() for t in S.make_episode(cfg, seed=11, noise_ratio=noise)[0][:4]]
        _cache[name] = (m, cfg, ep, ev)
    return _cache[name]


def _forward(m, ev, sx, sy, qx, qy, lp_iters=None):
    """forward() on one episode -> (logits, loss), cloned (MPTI's outputs live in buffers the next call reuses)."""
    with torch.no_grad():
        if hasattr(m, "lp_converged"):
            out = m(sx, sy, qx, qy, eval=ev, lp_iters=lp_iters)
            assert m.lp_converged()
        else:
            out = m(sx, sy, qx, qy)
    return out[0].clone(), out[1].clone()


def _fit_predict(m, ev, sx, sy, qx, qy, lp_iters=None):
    with torch.no_grad():
        f = m.fit_support(sx, sy, eval=ev, lp_iters=lp_iters)
        logits, loss = m.predict(f, qx, qy, lp_iters=lp_iters)
    if hasattr(m, "lp_converged"):
        assert m.lp_converged()
    return f, logits.clone(), loss.clone()


def _schedules(name):
    return [None, _model(name)[0].lp_max_iter] if name in MPTI else [None]


# ---- 1. bit equality with forward() ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_fit_then_predict_is_forward_bit_for_bit(name):
    m, cfg, (sx, sy, qx, qy), ev = _model(name)
    for lp_iters in _schedules(name):
        want_logits, want_loss = _forward(m, ev, sx, sy, qx, qy, lp_iters)
        f, logits, loss = _fit_predict(m, ev, sx, sy, qx, qy, lp_iters)
        assert torch.isfinite(want_logits).all()
        assert logits.shape == (qx.shape[0], cfg["n_way"] + 1, cfg["pc_npts"]) and loss.dim() == 0
        assert torch.equal(logits, want_logits), (name, lp_iters, (logits - want_logits).abs().max().item())
        assert torch.equal(loss, want_loss), (name, lp_iters, loss.item(), want_loss.item())
        if name in ("contrast", "mpti_eval"):  # the detection ran and dropped at least one shot
            keep = f.shot_keep.cpu()
            assert keep.numel() == cfg["n_way"] * cfg["k_shot"] and int((keep == 0).sum()) >= 1
        else:
            assert f.shot_keep is None
        if name == "mpti_fps":  # FPS really subsamples: a segment holds more points than prototypes
            d = f.head.desc.cpu()
            assert int(d[0]) > 21 and int(d[8]) in (20, 21)
        if name == "mpti_4way":
            assert f.head.Y.shape[0] == 2 * f.head.label_rows  # two label planes


# ---- 2. groups --------------------------------------------------------------------------------------------------------
def _groups(cfg, G=3):
    return [[t.cuda() for t in S.make_episode(cfg, seed=40 + g)[0][2:4]] for g in range(G)]


@pytest.mark.parametrize("name", ["proto_cos", "contrast", "mpti_fps", "mpti_4way"])
def test_groups_in_one_launch_sequence_equal_single_calls(name):
    m, cfg, (sx, sy, _, _), ev = _model(name)
    gs = _groups(cfg)
    QX, QY = torch.stack([g[0] for g in gs]), torch.stack([g[1] for g in gs])
    with torch.no_grad():
        f = m.fit_support(sx, sy, eval=ev)
        singles = []
        for qx, qy in gs:
            lo, ls = m.predict(f, qx, qy)
            singles.append((lo.clone(), ls.clone()))
        logits, loss = m.predict(f, QX, QY)
    assert logits.shape == (3,) + tuple(singles[0][0].shape) and loss.shape == (3,)
    for g in range(3):
        assert torch.equal(logits[g], singles[g][0]) and torch.equal(loss[g], singles[g][1]), (name, g)
    if name in MPTI:
        from r3dfsseg_amd.batch import EpisodeBatch
        assert m.lp_converged()
        logits, loss = logits.clone(), loss.clone()
        b = EpisodeBatch.from_episodes([[sx, sy, qx, qy] for qx, qy in gs])
        with torch.no_grad():
            want_logits, want_loss = m.forward_episodes(b, eval=ev)
        assert m.lp_converged()
        assert torch.equal(logits, want_logits) and torch.equal(loss, want_loss)


# ---- 3. the cache really is a cache -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proto_cos", "contrast", "mpti_eval"])
def test_predict_needs_nothing_of_the_support_set_after_the_fit(name):
    m, cfg, (sx, sy, qx, qy), ev = _model(name)
    want_logits, want_loss = _forward(m, ev, sx, sy, qx, qy)
    sx2, sy2 = sx.clone(), sy.clone()
    with torch.no_grad():
        f = m.fit_support(sx2, sy2, eval=ev)
    sx2.copy_(torch.rand_like(sx2) * 3 - 1)  # other clouds, other masks, in the memory the fit read
    sy2.copy_(1 - sy2)
    m._trace = None
    del sx2, sy2
    gc.collect()
    torch.cuda.empty_cache()  # whatever the fit no longer references goes back to the driver
    junk = torch.full((64 << 20,), float("nan"), device="cuda")  # ... and what the allocator hands out next is NaN
    del junk
    with torch.no_grad():
        logits, loss = m.predict(f, qx, qy)
    assert torch.equal(logits, want_logits) and torch.equal(loss, want_loss)


# ---- 4. n_q differs from n_way ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proto_cos", "contrast", "mpti_fps"])
def test_one_query_cloud_against_a_two_way_fit(name):
    m, cfg, (sx, sy, qx, qy), ev = _model(name)
    q1, y1 = qx[1:2], qy[1:2]
    want_logits, want_loss = _forward(m, ev, sx, sy, q1, y1)
    _, logits, loss = _fit_predict(m, ev, sx, sy, q1, y1)
    assert logits.shape == (1, cfg["n_way"] + 1, cfg["pc_npts"]) and loss.dim() == 0
    assert torch.equal(logits, want_logits) and torch.equal(loss, want_loss)
    with torch.no_grad():
        f = m.fit_support(sx, sy, eval=ev)
        lo, ls = m.predict(f, q1)
    assert ls is None and torch.equal(lo, want_logits)


# ---- 5. errors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["proto_cos", "mpti_fps"])
def test_shape_mode_and_stale_fit_errors(name):
    m, cfg, (sx, sy, qx, qy), ev = _model(name)
    with torch.no_grad():
        f = m.fit_support(sx, sy, eval=ev)
        with pytest.raises(ValueError, match="do not match the fit"):
            m.predict(f, qx[:, :, :-1])
        with pytest.raises(ValueError, match="do not match the fit"):
            m.predict(f, qx[:, :-1])
        with pytest.raises(ValueError, match="support_x"):
            m.fit_support(sx[..., :-1], sy)
        m.train()
        try:
            with pytest.raises(NotImplementedError):
                m.fit_support(sx, sy)
            with pytest.raises(NotImplementedError):
                m.predict(f, qx)
        finally:
            m.eval()
        m.predict(f, qx, qy)  # still good
        p = next(m.parameters())
        p.data.add_(1e-3)
        try:
            with pytest.raises(ValueError, match="stale fit"):
                m.predict(f, qx, qy)
        finally:
            p.data.sub_(1e-3)
            _cache.pop(name)  # (a + 1e-3 - 1e-3 is not a: the next test gets a fresh model)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_new_entry_points_refuse_null_pointers_and_short_buffers():
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()  # noqa: E731
    D, n_way, nq, cap = 64, 2, 128, 9
    f32 = dict(device="cuda", dtype=torch.float32)
    i32 = dict(device="cuda", dtype=torch.int32)
    fit_nodes, fit_Y, fit_desc = torch.zeros(cap, D, **f32), torch.zeros(cap, 4, **f32), torch.zeros(32, **i32)
    q = torch.zeros(nq, D, **f32)
    n_cap = cap + nq
    nodes, Y, desc = torch.zeros(n_cap, D, **f32), torch.zeros(n_cap, 4, **f32), torch.zeros(32, **i32)

    def attach(fit_nodes_, n_cap_):
        return lib.r3d_head_attach_queries_batched(1, _p(fit_nodes_), D, _p(fit_Y), cap, _p(fit_desc), None, cap, _p(q), D, nq,
                                                   n_way, D, nq, _p(nodes), D, n_cap_, _p(Y), _p(desc), 32, None, 0, None)
    assert attach(None, n_cap) != 0 and "r3d_head_attach_queries_batched" in err() and "null" in err()
    assert attach(fit_nodes, n_cap - 1) != 0 and "r3d_head_attach_queries_batched" in err() and "n_cap" in err()
    assert attach(fit_nodes, n_cap) == 0
    torch.cuda.synchronize()
    assert desc.tolist()[24:26] == [0, nq]  # an empty fit: no prototype rows, the query rows at the front

    sy = torch.zeros(2, 64, **i32)
    sf = torch.zeros(2 * 64, D, **f32)
    words = lib.r3d_protonet_head_ws_words(1, 2, 1)
    ws, protos = torch.zeros(words, **f32), torch.zeros(3, D, **f32)
    rc = lib.r3d_protonet_prototypes_batched(1, _p(sf), D, 0, D, _p(sy), None, 2, 1, 64, None, _p(ws), words, None)
    assert rc != 0 and "r3d_protonet_prototypes_batched" in err()
    rc = lib.r3d_protonet_prototypes_batched(1, _p(sf), D, 0, D, _p(sy), None, 2, 1, 64, _p(protos), _p(ws), words - 1, None)
    assert rc != 0 and "r3d_protonet_prototypes_batched" in err() and "workspace" in err()
    Z = torch.zeros(nq, 4, **f32)
    rc = lib.r3d_protonet_similarity_batched(1, _p(q), D, nq, D, None, 0, 2, nq, 0, 10.0, _p(Z), None)
    assert rc != 0 and "r3d_protonet_similarity_batched" in err()
    rc = lib.r3d_protonet_similarity_batched(2, _p(q), D, nq, D, _p(protos), D, 2, nq // 2, 0, 10.0, _p(Z), None)
    assert rc != 0 and "r3d_protonet_similarity_batched" in err() and "stride" in err()


def test_the_two_protonet_calls_are_the_fused_head_bit_for_bit():
    """The halves against r3d_protonet_head_keep_batched on given features: per-system tables and one broadcast table."""
    from r3dfsseg_amd import ops
    gen = torch.Generator().manual_seed(5)
    E, n_way, k_shot, N, n_q, D = 3, 5, 2, 96, 2, 100
    Sn, n_pts = n_way * k_shot, n_q * N
    ep_rows = Sn * N + n_pts + 3
    feat = (torch.randn(E * ep_rows, D + 4, generator=gen) + 0.5).cuda()[:, 4:]
    sy = (torch.rand(E, n_way, k_shot, N, generator=gen) < 0.3).to(torch.int32).cuda()
    keep = torch.ones(E, Sn, dtype=torch.int32)
    keep[:, 1] = 0
    keep = keep.cuda()
    for method in ("cosine", "euclidean"):
        want = ops.protonet_head_batched(feat[:Sn * N], feat[Sn * N:], sy, n_way, k_shot, N, method, E, ep_rows, n_pts, shot_keep=keep)
        protos = ops.protonet_prototypes(feat[:Sn * N], sy, n_way, k_shot, N, E, ep_rows, shot_keep=keep)
        assert protos.shape == (E, n_way + 1, D)
        got = ops.protonet_similarity(feat[Sn * N:], protos, n_way, method, E, n_pts, q_sys_rows=ep_rows)
        assert torch.isfinite(want).all() and torch.equal(got, want)
        one = ops.protonet_similarity(feat[Sn * N:], protos[1].contiguous(), n_way, method, E, n_pts, q_sys_rows=ep_rows)
        assert torch.equal(one.view(2, E, n_pts, 4)[:, 1], want.view(2, E, n_pts, 4)[:, 1])


# ---- 6. learners ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["mpti", "proto", "contrast"])
def test_learner_fit_then_predict_is_test(which):
    if which == "mpti":
        from r3dfsseg_amd.mpti_learner import MPTILearner_V3 as L
        cfg, noise, ev = S.make_cfg(n_way=2, k_shot=2, pc_npts=512, n_subprototypes=20), 0.0, True
    elif which == "proto":
        from r3dfsseg_amd.proto_learner import ProtoLearner as L
        cfg, noise, ev = S.make_cfg(n_way=2, k_shot=1, pc_npts=512), 0.0, False
    else:
        from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner as L
        cfg, noise, ev = S.make_cfg(n_way=2, k_shot=5, pc_npts=512), 0.4, False
    learner = L(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
    data = [t.cuda() for t in S.make_episode(cfg, seed=21, noise_ratio=noise)[0]]
    if which == "mpti":
        want = learner.test(data, None, eval=ev)
    else:
        want = learner.test(data, None)
    want = (want[0].clone(), want[1].clone(), want[2])
    f = learner.fit(data, eval=ev)
    assert learner.fitted is f
    pred, loss, acc = learner.predict(data[2], data[3])
    assert pred.dtype == want[0].dtype and torch.equal(pred, want[0]) and torch.equal(loss, want[1]) and acc == want[2]
    # a pair instead of an episode list, two groups, no labels
    f2 = learner.fit((data[0], data[1]), eval=ev)
    res = learner.predict(torch.stack([data[2], data[2]]), fitted=f2)
    assert len(res) == 2 and all(torch.equal(r[0], want[0]) and r[1] is None and r[2] is None for r in res)
