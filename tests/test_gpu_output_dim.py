"""Attention at head widths 32, 96, 128 (the reference's --output_dim): the kernels of both matrix arithmetics against
the reference's own SelfAttention (tests/golden/attention_d*.npz, tools/gen_golden_attention_dims.py) and against a
float64 restatement, forward and backward, with and without dropout; the dropout mask is the same at every width and in
both arithmetics; then the models built at those widths, end to end."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from attn_ref import keep_mask as _keep_mask  # csrc/attention.hip::attn_keep for every (cloud, query, key)
from oracle import r3d_oracle as O
from r3dfsseg_amd import synthetic as S

pytestmark = pytest.mark.gpu
TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = (32, 96, 128)


def _rel(a, b):
    return ((a.double() - b).abs().max() / b.abs().max()).item()



def _ref(qkv, B, N, D, dO, keep=None, p_drop=0.0):
    """float64 restatement of models/attention.py:43-46 (q arrives scaled) and its gradient w.r.t. q | k | v."""
    q, k, v = (qkv[:, D * i:D * (i + 1)].double().cpu().view(B, N, D) for i in range(3))
    P = torch.softmax(q @ k.transpose(1, 2), -1)
    sc = keep.double() / (1.0 - float(np.float32(p_drop))) if keep is not None else 1.0
    Pd = P * sc
    out = (Pd @ v).reshape(B * N, D)
    g = dO.double().cpu().view(B, N, D)
    dV = Pd.transpose(1, 2) @ g
    dP = (g @ v.transpose(1, 2)) * sc
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    return out, torch.cat((dS @ k, dS.transpose(1, 2) @ q, dV), -1).reshape(B * N, 3 * D)


def _run(lib, mode, qkv, B, N, D, dO, p_drop=0.0, seed=0):
    """forward + backward at head width D in arithmetic `mode` (0 fp32, 1 bf16 x 3); the backward once on the
    forward's workspace (packed q | k | v reused) and once cutting them again: both must agree bit for bit."""
    from r3dfsseg_amd import _lib
    from r3dfsseg_amd.ops import _p, _st
    before = lib.r3d_get_matrix_arith()
    _lib.check(lib.r3d_set_matrix_arith(mode))
    try:
        ws = torch.empty(lib.r3d_attention_ws_words_ep_d(B, N, 0, D), device="cuda")
        out = torch.empty(B * N, D, device="cuda")
        lse = torch.empty(B * N, device="cuda")
        dqkv = torch.empty(B * N, 3 * D, device="cuda")
        dqkv2 = torch.empty_like(dqkv)
        _lib.check(lib.r3d_attention_fwd_train_ep_d(_p(qkv), 3 * D, B, N, _p(out), D, _p(lse), p_drop, seed, None, 0, D,
                                                    _p(ws), _st()))
        _lib.check(lib.r3d_attention_bwd_ep_d(_p(qkv), 3 * D, B, N, _p(out), D, _p(dO), D, _p(lse), p_drop, seed, None, 0, D,
                                              1.0, _p(dqkv), 3 * D, _p(ws), 1, _st()))
        _lib.check(lib.r3d_attention_bwd_ep_d(_p(qkv), 3 * D, B, N, _p(out), D, _p(dO), D, _p(lse), p_drop, seed, None, 0, D,
                                              1.0, _p(dqkv2), 3 * D, _p(ws), 0, _st()))
        torch.cuda.synchronize()
        assert torch.equal(dqkv, dqkv2)
    finally:
        _lib.check(lib.r3d_set_matrix_arith(before))
    return out, dqkv


def _inputs(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * D, generator=g)
    qkv[:, :D] *= 0.5 * (64.0 / D) ** 0.5  # scores of the D = 64 tests' spread
    dO = torch.randn(B * N, D, generator=g)
    return qkv.cuda(), dO.cuda()


@pytest.mark.parametrize("D", WIDTHS)
def test_attention_module_against_the_reference(D):
    """dgcnn.SelfAttention(256, D) in eval mode on the reference's inputs and weights, both arithmetics."""
    from r3dfsseg_amd import _lib
    from r3dfsseg_amd.dgcnn import SelfAttention
    lib = _lib.load()
    z = np.load(os.path.join(GOLDEN, "attention_d%d.npz" % D))
    att = SelfAttention(256, D)
    att.load_state_dict({"%s_map.weight" % m: torch.from_numpy(z["w" + m]) for m in "qkv"})
    att = att.cuda().eval()
    want = torch.from_numpy(z["y"]).double()
    before = lib.r3d_get_matrix_arith()
    try:
        for mode in (0, 1):
            _lib.check(lib.r3d_set_matrix_arith(mode))
            with torch.no_grad():
                y = att(torch.from_numpy(z["x"]).cuda()).cpu()
            assert y.shape == want.shape
            assert (y.double() - want).abs().max().item() <= TOL, (mode, (y.double() - want).abs().max().item())
    finally:
        _lib.check(lib.r3d_set_matrix_arith(before))


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B,N", [(2, 512), (2, 500)])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_attention_forward_backward_against_float64(D, B, N, p_drop):
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    qkv, dO = _inputs(B, N, D, 1000 * D + N)
    seed = 4321
    keep = _keep_mask(B, N, seed, p_drop) if p_drop > 0 else None
    want, want_d = _ref(qkv, B, N, D, dO, keep, p_drop)
    for mode in (0, 1):
        out, dqkv = _run(lib, mode, qkv, B, N, D, dO, p_drop, seed)
        assert _rel(out.cpu(), want) <= TOL, (mode, _rel(out.cpu(), want))
        for i in range(3):
            err = _rel(dqkv[:, D * i:D * (i + 1)].cpu(), want_d[:, D * i:D * (i + 1)])
            assert err <= TOL, (mode, "qkv"[i], err)


def test_dropout_mask_is_the_same_at_every_width_and_in_both_arithmetics():
    """v = identity columns: the output then IS the dropped attention matrix restricted to D keys, so the kernels' own
    mask is read off directly and compared with the hash and across widths / arithmetics."""
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    B, N, p, seed = 2, 256, 0.1, 99
    masks = []
    for D in (32, 64, 96, 128):
        qkv = torch.zeros(B * N, 3 * D)
        qkv[:, 2 * D:] = torch.eye(N, D).repeat(B, 1)  # v[key] = e_key for the first D keys, 0 beyond
        qkv = qkv.cuda()                                 # q = k = 0: uniform weights 1 / N
        dO = torch.zeros(B * N, D, device="cuda")
        for mode in (0, 1):
            out, _ = _run(lib, mode, qkv, B, N, D, dO, p, seed)
            masks.append((out.cpu().view(B, N, D)[..., :32] > 0))
    want = _keep_mask(B, N, seed, p)[..., :32]
    for m in masks:
        assert torch.equal(m, want)


@pytest.mark.parametrize("D", WIDTHS)
def test_attention_is_deterministic(D):
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    qkv, dO = _inputs(3, 700, D, 7)
    for mode in (0, 1):
        a = _run(lib, mode, qkv, 3, 700, D, dO, 0.1, 5)
        b = _run(lib, mode, qkv, 3, 700, D, dO, 0.1, 5)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_unsupported_width_is_refused_before_a_launch():
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    assert lib.r3d_attention_ws_words_ep_d(2, 128, 0, 48) == -1
    qkv = torch.zeros(256, 144, device="cuda")
    out = torch.zeros(256, 48, device="cuda")
    lse = torch.zeros(256, device="cuda")
    from r3dfsseg_amd.ops import _p, _st
    assert lib.r3d_attention_fwd_train_ep_d(_p(qkv), 144, 2, 128, _p(out), 48, _p(lse), 0.0, 0, None, 0, 48, None, _st()) != 0
    assert "head width 48" in lib.r3d_last_error_string().decode()


def _close(got, want):
    return ((got - want).abs() / want.abs().clamp(min=1.0)).max().item()


@pytest.mark.parametrize("D", [32, 128])
def test_mpti_eval_logits_against_the_oracle(D):
    """2-way 2-shot at 512 points: features (neighbour lists injected) and logits (on the device's node matrix) within
    1e-4 of the oracle's float64 / fp32 restatement, as tests/test_gpu_parity_full.py does at 64."""
    from r3dfsseg_amd.mpti import MPTI_SelfAtten
    cfg = S.make_cfg(n_way=2, k_shot=2, pc_npts=512, output_dim=D)
    sd = S.make_state_dict(cfg, 123)
    m = MPTI_SelfAtten(SimpleNamespace(**cfg))
    m.load_state_dict(sd)
    m = m.cuda().eval()
    data, _ = S.make_episode(cfg, seed=78)
    sx, sy, qx, qy = data[:4]
    n_way, k_shot, N = cfg["n_way"], cfg["k_shot"], cfg["pc_npts"]
    Sn = n_way * k_shot
    m._trace = {}
    with torch.no_grad():
        logits, loss = m(sx.cuda(), sy.cuda(), qx.cuda(), qy.cuda(), lp_iters=m.lp_max_iter)
    assert m.lp_converged()
    tr, hb = m._trace, m._head[1]
    x_all = torch.cat((sx.reshape(Sn, 9, N), qx), 0)
    B = x_all.shape[0]
    idx_hip = [i.cpu().to(torch.int64) for i in tr["idx"][0]]
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    feat_ref = O.get_features(sd64, x_all.double(), cfg, idx_override=idx_hip)
    feat_hip = torch.cat((tr["sfeat"], tr["qfeat"]), 0).cpu().reshape(B, N, -1).transpose(1, 2)
    assert feat_hip.shape[1] == 64 + D + 64
    assert _close(feat_hip.double(), feat_ref) <= TOL, _close(feat_hip.double(), feat_ref)
    from r3dfsseg_amd import ops
    n_proto = int(hb.desc[0, ops.HD_N_PROTO].item())
    n = int(hb.desc[0, ops.HD_N_NODES].item())
    nodes = hb.nodes[:n].cpu()
    A = O.affinity(nodes, cfg["k_connect"], cfg["sigma"])
    Zo = O.label_propagate(A, hb.Y[:n, :n_way + 1].cpu(), dtype=torch.float64)
    want_logits = Zo[n_proto:].view(-1, N, n_way + 1).transpose(1, 2)
    assert _close(logits.cpu().double(), want_logits) <= TOL, _close(logits.cpu().double(), want_logits)


def _learner(cfg, mode):
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    L = MPTILearner_V3(SimpleNamespace(**cfg), mode=mode)
    L.model.att_learner.dropout.p = 0.0
    L.model._lp_budget = 150
    return L


@pytest.mark.parametrize("D", [32, 128])
def test_test_batch_equals_the_conservative_eager_schedule(D):
    cfg = S.make_cfg(n_way=2, k_shot=2, pc_npts=512, output_dim=D, pretrain_checkpoint_path=None,
                     model_checkpoint_path="synthetic")
    L = _learner(cfg, "test")
    eps = []
    for e in range(3):
        data, _ = S.make_episode(cfg, seed=60 + e, noise_ratio=0.5)
        eps.append([t.cuda() for t in data])
    got = L.test_batch(eps, None)
    for e, ep in enumerate(eps):
        with torch.no_grad():
            logits, loss = L.model(ep[0], ep[1], ep[2], ep[3], lp_iters=L.model.lp_max_iter)
        assert L.model.lp_converged()
        assert torch.equal(got[e][0], logits.argmax(1))  # logits (n_q, n_classes, N)
        assert abs(float(got[e][1]) - float(loss)) < 2e-5


def test_train_batch_at_output_dim_128():
    """One train_batch step (captured-graph batch path) against the same episodes run one at a time on the eager path:
    the attention and projection gradients agree within the bar of tests/test_gpu_learner_batch.py."""
    from r3dfsseg_amd.dp_train import DPTrainer
    cfg = S.make_cfg(n_way=2, k_shot=2, pc_npts=512, output_dim=128, pretrain_checkpoint_path="synthetic",
                     model_checkpoint_path=None, lr=1e-3, step_size=5000, gamma=0.5)
    eps = []
    for e in range(2):
        data, _ = S.make_episode(cfg, seed=40 + e, noise_ratio=0.5, train=True)
        eps.append([t.cuda() for t in data])
    A, Bm = _learner(cfg, "train"), _learner(cfg, "train")
    tr = DPTrainer(A)
    tr.step(eps)
    got = Bm.train_batch(eps, None)
    # the step ran as a captured hipGraph (a failed capture would have left the trainer on eager launches)
    bt = Bm._batch_trainer
    assert bt.batch_graph and bt.runner.__dict__.get("_graph") is not None
    assert len(got) == 2 and all(torch.isfinite(torch.as_tensor(float(o[0]))) for o in got)
    for e, (o, w) in enumerate(zip(got, tr.last_outputs)):
        assert abs(float(o[0]) - float(w[0])) < 2e-5
    names = [n for n, _ in A.model.named_parameters() if n.startswith(("att_learner.", "proj."))]
    assert "att_learner.q_map.weight" in names and "proj.weight" in names
    pa, pb = dict(A.model.named_parameters()), dict(Bm.model.named_parameters())
    ga = torch.cat([pa[n].grad.reshape(-1) for n in names])
    gb = torch.cat([pb[n].grad.reshape(-1) for n in names])
    assert ga.abs().max().item() > 0
    assert (ga - gb).abs().max().item() <= 2e-6 * ga.abs().max().item()
    assert tuple(pa["att_learner.q_map.weight"].shape) == (128, 256, 1) and tuple(pa["proj.weight"].shape) == (128, 256)
    # the reference's attention dropout (p = 0.1) inside the replayed graph at D = 128: the same graph replays, the step
    # stays finite and solvable (its numbers against float64 with the mask injected: test_encoder_train_at_output_dim_128)
    Bm.model.att_learner.dropout.p = 0.1
    g0 = bt.runner.__dict__.get("_graph")
    got = Bm.train_batch(eps, None)
    assert bt.batch_graph and bt.runner.__dict__.get("_graph") is g0
    assert all(np.isfinite(float(o[0])) for o in got)
    assert all(torch.isfinite(p.grad).all() for p in Bm.model.parameters() if p.grad is not None)


@pytest.mark.parametrize("use_attention", [True, False])
def test_protonet_at_output_dim_32(use_attention):
    from r3dfsseg_amd.protonet import ProtoNet
    cfg = S.make_cfg(n_way=2, k_shot=1, pc_npts=512, output_dim=32, use_attention=use_attention)
    sd = S.make_state_dict(cfg, 123)
    sd = {k: v for k, v in sd.items() if not k.startswith("proj.")}
    m = ProtoNet(SimpleNamespace(**cfg))
    m.load_state_dict(sd)
    m = m.cuda().eval()
    data, _ = S.make_episode(cfg, seed=5)
    sx, sy, qx, qy = data[:4]
    with torch.no_grad():
        logits, loss = m(sx.cuda(), sy.cuda(), qx.cuda(), qy.cuda())
        feat = m.getFeatures(torch.cat((sx.reshape(-1, 9, 512), qx), 0).cuda()).cpu()
    assert feat.shape[1] == 64 + 32 + 64
    # the head restated in float64 (models/protonet.py, oracle.protonet_forward) on the device's own features
    f64 = feat.double()
    Sn = cfg["n_way"] * cfg["k_shot"]
    sfeat, qfeat = f64[:Sn].view(cfg["n_way"], cfg["k_shot"], -1, 512), f64[Sn:]
    syd = sy.double().unsqueeze(2)

    def masked(f, m):
        return (f * m).sum(3) / (m.sum(3) + 1e-5)
    fg, bg = masked(sfeat, syd), masked(sfeat, 1.0 - syd)
    protos = [bg.sum(dim=(0, 1)) / Sn] + [fg[w].sum(0) / cfg["k_shot"] for w in range(cfg["n_way"])]
    want_logits = torch.stack([torch.nn.functional.cosine_similarity(qfeat, p[None, :, None], dim=1) * 10 for p in protos], 1)
    want_loss = torch.nn.functional.cross_entropy(want_logits, qy)
    assert _close(logits.cpu().double(), want_logits) <= TOL, _close(logits.cpu().double(), want_logits)
    assert abs(loss.item() - want_loss.item()) <= TOL, (loss.item(), want_loss.item())
    # the attention / linear columns on their own, against float64 on the device's own encoder output
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x_all = torch.cat((sx.reshape(-1, 9, 512), qx), 0)
    idx = [i.cpu().to(torch.int64) for i in _encoder_idx(m, x_all)]
    feat_ref = O.get_features(sd64, x_all.double(), cfg, idx_override=idx)
    assert _close(feat.double(), feat_ref) <= TOL, _close(feat.double(), feat_ref)


def _encoder_idx(m, x):
    """The encoder's neighbour lists on x (the parity tests' trace hook)."""
    from r3dfsseg_amd import ops
    B, _, N = x.shape
    m.encoder.trace = []
    with torch.no_grad():
        x_pm, x_cm = ops.input_layouts(x.cuda())
        m.encoder.forward_pm(x_pm, B, N, x_cm=x_cm)
    idx = m.encoder.trace
    m.encoder.trace = None
    return idx


def test_encoder_train_at_output_dim_128():
    """getFeatures in training mode at output_dim = 128 (feature width 256) with the reference's attention dropout on,
    against torch autograd through the oracle in float64: neighbour lists, max-pool winners AND the kernels' dropout keep
    mask injected.  Every slice of the training path that depends on the width is on this road: the base learner's
    columns, the (M, 3 D) q | k | v, the split of dWqkv into the three maps, the input gradient through them.  Bars of
    tests/test_gpu_train.py::test_encoder_train_forward_and_gradients: features 1e-4, every gradient 2e-3 rel-L2."""
    from r3dfsseg_amd import train_ops as T
    from r3dfsseg_amd.mpti import MPTI_SelfAtten
    B, N, D, p, seed = 2, 512, 128, 0.1, 7
    cfg = S.make_cfg(n_way=2, k_shot=1, pc_npts=N, output_dim=D)
    sd = S.make_state_dict(cfg, 123, feat_scale=1.0)
    m = MPTI_SelfAtten(SimpleNamespace(**cfg))
    m.load_state_dict(sd)
    m.cuda().train()
    m.att_learner.dropout.p = p
    assert m._slot.seed_dev is None  # eager: the mask is the one of `seed` itself
    F = m.feat_dim
    assert F == 256
    pc = torch.from_numpy(np.stack([S._cloud(np.random.RandomState(90 + i), N, 0.0).T for i in range(B)]).copy())
    R = torch.from_numpy(np.random.RandomState(5).randn(B * N, F).astype(np.float32))
    m._trace = {}
    feat = T.get_features_train(m, pc.cuda(), seed=seed)
    (feat * R.cuda()).sum().backward()
    idx = [i.cpu().to(torch.int64) for i in m._trace["idx"][0]]
    am = [a.cpu().to(torch.int64).view(B, N, 64).permute(0, 2, 1).contiguous() for a in m._trace["argmax"][0]]
    m._trace = None
    keep = _keep_mask(B, N, seed, p).double() / (1.0 - float(np.float32(p)))
    assert 0.08 < 1.0 - (keep > 0).double().mean().item() < 0.12
    sdr = {k: (v.double().requires_grad_() if v.dtype.is_floating_point and "running" not in k
               else (v.double() if v.dtype.is_floating_point else v.clone())) for k, v in sd.items()}
    ns = {}
    fo = O.get_features(sdr, pc.double(), cfg, train=True, new_stats=ns, drop_mask=keep, idx_override=idx,
                        argmax_override=am)
    fo_pm = fo.transpose(1, 2).reshape(B * N, F)
    d = ((feat.detach().cpu().double() - fo_pm.detach()).abs() / fo_pm.detach().abs().clamp(min=1.0)).max().item()
    assert d <= TOL, d
    (fo_pm * R.double()).sum().backward()
    worst = []
    for name, prm in m.named_parameters():
        if name.startswith("proj."):
            continue
        gref = sdr[name].grad
        assert prm.grad is not None, name
        if name.startswith("base_learner") and name.endswith(".0.bias"):
            assert prm.grad.abs().max().item() < 1e-3 and gref.abs().max().item() < 1e-3
            continue
        g = prm.grad.cpu().double()
        worst.append((((g - gref).norm() / gref.norm()).item(), name))
    names = [n for _, n in worst]
    assert all("att_learner.%s_map.weight" % c in names for c in "qkv")
    print("gradient errors (rel-L2):", sorted(worst)[-4:])
    assert max(e for e, _ in worst) <= 2e-3, sorted(worst)[-4:]


_SPLIT_CHECK = r"""
import sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_output_dim as T
from r3dfsseg_amd import _lib
lib = _lib.load()
for D in (32, 96, 128):
    for B, N in ((2, 500), (3, 1000)):
        qkv, dO = T._inputs(B, N, D, 31 * D + N)
        keep = T._keep_mask(B, N, 11, 0.1)
        want, want_d = T._ref(qkv, B, N, D, dO, keep, 0.1)
        for mode in (0, 1):
            out, dqkv = T._run(lib, mode, qkv, B, N, D, dO, 0.1, 11)
            e = max([T._rel(out.cpu(), want)] + [T._rel(dqkv[:, D * i:D * (i + 1)].cpu(), want_d[:, D * i:D * (i + 1)])
                                                  for i in range(3)])
            print(D, B, N, mode, e)
            assert e <= T.TOL, (D, B, N, mode, e)
print("SPLIT_OK")
"""


def test_key_axis_split_at_other_widths():
    """The streamed-axis split (R3D_ATT_SPLIT, read once per process: a child process) at D = 32, 96, 128: partials of
    [split][M][D + 4] merged by the combine kernel, dK | dV partials of [split][M][2 D] and dQ partials of [split][M][D]
    summed into their columns -- against float64 with dropout, both arithmetics."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = _SPLIT_CHECK % {"root": os.path.dirname(here), "tests": here}
    env = dict(os.environ, R3D_ATT_SPLIT="3")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SPLIT_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
