"""ProtoNet_Contrast on the device: r3d_protonet_head_keep_batched (the ProtoNet head that honours shot_keep) and the
model / learner around it.

Bars.  Keep-all against the plain head, a batch against its episodes, test_batch against test(): torch.equal.  The head
against the float64 restatement (tests/protonet_contrast_ref.py) on the SAME features: |diff| <= 1e-3 * max(1, max|want|),
the number tests/test_gpu_aux.py holds the ProtoNet head to -- there with 3 % of the points excused for kNN near-ties in the
encoder; here the features are given, so every point must meet it.

The whole model: against the reference's own ProtoNet_Contrast on the stored 2-way 5-shot episode (tests/golden/
protonet_contrast.npz; for 5-way 2-shot no episode can be stored with inputs, tools/gen_golden_protonet_contrast.py says
why), and for 2-way 5-shot, 5-way 2-shot and 5-way 3-shot against the oracle's clean-shot detection and the restatement
on the device's own features, at the bars of tests/test_gpu_parity_full.py (1e-4)."""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from r3dfsseg_amd import synthetic as S  # noqa: E402
import protonet_contrast_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

N = 256


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _problem(E, n_way, k_shot, D, n_q, seed):
    """E episodes in one feature matrix (a column slice: leading dimension != D), [support rows | query rows | 19 NaN rows]
    each; every shot has foreground and background."""
    gen = torch.Generator().manual_seed(seed)
    Sn, n_pts = n_way * k_shot, n_q * N
    ep_rows = Sn * N + n_pts + 19
    buf = torch.randn(E * ep_rows, D + 7, generator=gen) + 0.5
    buf.view(E, ep_rows, D + 7)[:, Sn * N + n_pts:] = float("nan")
    sy = (torch.rand(E, n_way, k_shot, N, generator=gen) < 0.3).to(torch.int32)
    sy[..., 0] = 1
    sy[..., 1] = 0
    return buf.cuda()[:, 3:3 + D], sy.cuda(), ep_rows


def _head(feat, sy, keep, n_way, k_shot, n_q, method, E, ep_rows):
    from r3dfsseg_amd import ops
    Sn = n_way * k_shot
    Z = ops.protonet_head_batched(feat[:Sn * N], feat[Sn * N:], sy, n_way, k_shot, N, method, E, ep_rows, n_q * N, shot_keep=keep)
    return Z.view(1 if n_way <= 3 else 2, E, n_q * N, 4)


def _want(feat, sy, keep, n_way, k_shot, n_q, method, e, ep_rows):
    """The restatement on episode e's rows -> (n_q * N, n_way + 1) float64."""
    Sn, D = n_way * k_shot, feat.shape[1]
    rows = feat[e * ep_rows:(e + 1) * ep_rows].cpu()
    sf = rows[:Sn * N].view(n_way, k_shot, N, D).transpose(2, 3)
    qf = rows[Sn * N:Sn * N + n_q * N].view(n_q, N, D).transpose(1, 2)
    z = R.head(sf, sy[e].cpu(), qf, None if keep is None else keep[e].cpu(), method)  # (n_q, C, N)
    return z.transpose(1, 2).reshape(n_q * N, n_way + 1)


def _cols(Zv, e, n_classes):
    """(planes, E, n_pts, 4) -> (n_pts, n_classes) of episode e."""
    return torch.cat([Zv[p, e] for p in range(Zv.shape[0])], 1)[:, :n_classes]


@pytest.mark.parametrize("method", ["cosine", "euclidean"])
@pytest.mark.parametrize("D", [192, 100])
def test_keep_all_is_the_plain_head_bit_for_bit(D, method):
    from r3dfsseg_amd import _lib
    E, n_way, k_shot, n_q = 3, 2, 5, 2
    Sn, n_pts = n_way * k_shot, n_q * N
    feat, sy, ep_rows = _problem(E, n_way, k_shot, D, n_q, 700 + D)
    lib = _lib.load()
    words = lib.r3d_protonet_head_ws_words(E, n_way, k_shot)
    ws = torch.empty(words, device="cuda")
    plain = torch.empty(E * n_pts, 4, device="cuda")
    sy32 = sy.reshape(E * Sn, N).contiguous()
    rc = lib.r3d_protonet_head_batched(E, _p(feat), feat.stride(0), _p(feat[Sn * N:]), feat.stride(0), ep_rows, D, _p(sy32), n_way,
                                       k_shot, N, n_pts, 0 if method == "cosine" else 1, 10.0, _p(plain), _p(ws), words, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(plain).all()
    none = _head(feat, sy, None, n_way, k_shot, n_q, method, E, ep_rows)
    ones = _head(feat, sy, torch.ones(E, Sn, dtype=torch.int32, device="cuda"), n_way, k_shot, n_q, method, E, ep_rows)
    assert torch.equal(none.reshape(-1, 4), plain) and torch.equal(ones.reshape(-1, 4), plain)


def _patterns(E, n_way, k_shot):
    one = torch.ones(E, n_way, k_shot, dtype=torch.int32)
    a = one.clone(); a[:, 0, 1] = 0                       # one shot dropped
    b = torch.zeros_like(one); b[:, :, k_shot - 1] = 1    # all but one dropped, in every way
    c = one.clone()                                       # another pattern per episode
    for e in range(E):
        c[e, e % n_way, e % k_shot] = 0
        c[e, (e + 1) % n_way, (e + 1) % k_shot] = 0
    return [a, b, c]


@pytest.mark.parametrize("method", ["cosine", "euclidean"])
@pytest.mark.parametrize("n_way,k_shot", [(2, 5), (5, 2)])
def test_keep_head_against_the_restatement(n_way, k_shot, method):
    E, n_q, D = 2, 1, 192
    feat, sy, ep_rows = _problem(E, n_way, k_shot, D, n_q, 800 + n_way)
    for keep in _patterns(E, n_way, k_shot):
        kd = keep.reshape(E, -1).cuda()
        Z = _head(feat, sy, kd, n_way, k_shot, n_q, method, E, ep_rows)
        assert torch.isfinite(Z).all()
        for e in range(E):
            want = _want(feat, sy, keep, n_way, k_shot, n_q, method, e, ep_rows)
            got = _cols(Z, e, n_way + 1).cpu().double()
            err, bar = float((got - want).abs().max()), 1e-3 * max(1.0, float(want.abs().max()))
            print("%d-way %d-shot %s episode %d: max |diff| %.3e (bar %.3e)" % (n_way, k_shot, method, e, err, bar))
            assert err <= bar
            if n_way > 3:  # the unused columns of plane 1 are zero
                assert not Z[1, e][:, n_way + 1 - 4:].any()
            # the episode alone, through a batch of one: the same bits
            rows = feat[e * ep_rows:(e + 1) * ep_rows]
            Z1 = _head(rows, sy[e], kd[e], n_way, k_shot, n_q, method, 1, 0)
            assert torch.equal(Z1[:, 0], Z[:, e])


def test_a_dropped_shot_feeds_the_background_only():
    E, n_way, k_shot, n_q, D = 1, 2, 5, 1, 192
    feat, sy, ep_rows = _problem(E, n_way, k_shot, D, n_q, 900)
    keep = torch.ones(1, n_way * k_shot, dtype=torch.int32, device="cuda")
    keep[0, 3] = 0  # way 0, shot 3
    Z0 = _head(feat, sy, keep, n_way, k_shot, n_q, "cosine", E, ep_rows)
    fg = feat.clone()
    rows = fg[3 * N:4 * N]
    rows[sy[0, 0, 3] == 1] += 1.0   # its foreground rows
    Z1 = _head(fg, sy, keep, n_way, k_shot, n_q, "cosine", E, ep_rows)
    assert torch.equal(Z1, Z0)
    bgf = feat.clone()
    rows = bgf[3 * N:4 * N]
    rows[sy[0, 0, 3] == 0] += 1.0   # its background rows: the shot still counts there
    Z2 = _head(bgf, sy, keep, n_way, k_shot, n_q, "cosine", E, ep_rows)
    assert torch.equal(Z2[0, 0][:, 1:3], Z0[0, 0][:, 1:3]) and not torch.equal(Z2[0, 0][:, 0], Z0[0, 0][:, 0])
    # and a kept shot's foreground does move its way's column, and only that one
    rows = fg[2 * N:3 * N]
    rows[sy[0, 0, 2] == 1] += 1.0
    Z3 = _head(fg, sy, keep, n_way, k_shot, n_q, "cosine", E, ep_rows)
    assert not torch.equal(Z3[0, 0][:, 1], Z0[0, 0][:, 1]) and torch.equal(Z3[0, 0][:, 2], Z0[0, 0][:, 2])


def test_host_flags_without_a_kept_shot_are_refused():
    """ops.protonet_head_batched checks a HOST shot_keep before anything is launched (the device never checks its own)."""
    feat, sy, ep_rows = _problem(1, 2, 2, 64, 1, 950)
    with pytest.raises(ValueError, match="every shot of a way"):
        _head(feat, sy, torch.tensor([[1, 0, 0, 0]]), 2, 2, 1, "cosine", 1, 0)
    with pytest.raises(ValueError, match="entries"):
        _head(feat, sy, torch.tensor([[1, 0, 1]]), 2, 2, 1, "cosine", 1, 0)
    Z = _head(feat, sy, torch.tensor([[1, 0, 0, 1]]), 2, 2, 1, "cosine", 1, 0)  # a host tensor that is in order: uploaded
    assert torch.equal(Z, _head(feat, sy, torch.tensor([[1, 0, 0, 1]], dtype=torch.int32).cuda(), 2, 2, 1, "cosine", 1, 0))


def _learner(cfg):
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    return ProtoContrastLearner(SimpleNamespace(**dict(cfg, model_checkpoint_path='synthetic')), mode='test')


TOL = 1e-4  # tests/test_gpu_parity_full.py: values |got - want| / max(1, |want|), losses 1e-4 * max(1, |loss|), arg-max >= 0.99


def _close(got, want):
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max())


def _expected_keep(O, sf, sy, sx, k_shot):
    """The oracle's clean-shot flags on the given features.  Two shots per way: at scale (1,1,1) the two row sums of a way are
    ONE number in exact arithmetic, `sum > mean` is false for both on the device (it computes the two mirror entries alike)
    while a BLAS may round them apart; so that scale's flags are taken as 0 and the decision is the oracle's at scale
    (2,2,1) alone, where no tie arises: total = flag / 2 < 0.5 drops, a way with nothing left is reset to all kept."""
    if k_shot != 2:
        return O.mean_pl_support_y_multi_scale(sf, sy, sx)[1]
    _, flag = O.mean_pl_support_y(sf, sy, sx, 2, 2, 1)
    keep = (flag / 2 >= 0.5).float()
    keep[keep.sum(1) == 0] = 1.0
    return keep


# 5-way 3-shot: the second plane of label columns with a detection that has no structural tie
@pytest.mark.parametrize("n_way,k_shot", [(2, 5), (5, 2), (5, 3)])
def test_whole_model_against_the_oracle_detection_and_the_restatement(n_way, k_shot):
    from oracle import r3d_oracle as O
    from r3dfsseg_amd import ops
    cfg = S.make_cfg(n_way=n_way, k_shot=k_shot, n_queries=1, pc_npts=512)
    L = _learner(cfg)
    m = L.model.eval()
    eps = [S.make_episode(cfg, seed, noise_ratio=0.4)[0] for seed in (3, 4)]
    Sn, Np, n_q = n_way * k_shot, 512, n_way
    dropped = 0
    for data in eps:
        sx, sy, qx, qy = data[:4]
        m._trace = {}
        with torch.no_grad():
            logits, loss = m(sx.cuda(), sy.cuda(), qx.cuda(), qy.cuda())
        feat, keep = m._trace["feat"], m._trace["shot_keep"].cpu().view(n_way, k_shot)
        m._trace = None
        assert logits.shape == (n_q, n_way + 1, Np)
        fcm = ops.pm_to_cm(feat, Sn + n_q, Np).cpu()
        sf, qf = fcm[:Sn].view(n_way, k_shot, -1, Np), fcm[Sn:]
        want_keep = _expected_keep(O, sf, sy, sx, k_shot)
        assert torch.equal(keep.float(), want_keep), (keep, want_keep)
        assert (keep.sum(1) > 0).all()
        dropped += int((keep == 0).sum())
        want = R.head(sf, sy, qf, keep, "cosine")
        err = _close(logits.cpu().double(), want)
        wloss = float(F.cross_entropy(want, qy.long()))
        agree = float((logits.cpu().argmax(1) == want.argmax(1)).float().mean())
        print("%d-way %d-shot: dropped %d of %d shots, logits vs restatement %.3e, |loss - want| %.3e, arg-max agreement %.4f"
              % (n_way, k_shot, int((keep == 0).sum()), Sn, err, abs(float(loss) - wloss), agree))
        assert err <= TOL
        assert abs(float(loss) - wloss) <= TOL * max(1.0, abs(wloss))
        assert agree >= 0.99
    assert dropped > 0, "no shot was dropped in either episode: the keep path was not exercised"
    # test_batch over [ep, ep2, ep] against three test() calls: the same bits
    single = [L.test([t.cuda() for t in d], None, step=0, path=None, eval=True) for d in (eps[0], eps[1], eps[0])]
    batch = L.test_batch([eps[0], eps[1], eps[0]])
    for (p1, l1, a1), (p2, l2, a2) in zip(single, batch):
        assert torch.equal(p1, p2) and torch.equal(l1, l2) and a1 == a2
    assert torch.equal(batch[0][0], batch[2][0])


def test_whole_model_against_the_reference_fixture():
    """The reference's own ProtoNet_Contrast.forward(train=False) (tests/golden/protonet_contrast.npz, 2-way 5-shot, stored
    with its inputs because every `cosine_sum > mean` vote is 1e-2 clear): shot_keep equals its clean_flag exactly;
    query_pred and loss at the bars of tests/test_gpu_parity_full.py."""
    import numpy as np
    g = np.load(os.path.join(ROOT, "tests", "golden", "protonet_contrast.npz"))
    p = "w2k5/"
    assert int(g[p + "gpu_ok"]) == 1
    cfg = S.make_cfg(n_way=2, k_shot=5, n_queries=1, pc_npts=512)
    L = _learner(cfg)  # synthetic.make_state_dict(cfg, 123): the generator's weights
    m = L.model.eval()
    t = lambda k, dt=None: torch.from_numpy(g[p + k]).to(dt) if dt else torch.from_numpy(g[p + k])  # noqa: E731
    sx, sy, qx, qy = t("support_x"), t("support_y", torch.int32), t("query_x"), t("query_y", torch.int64)
    m._trace = {}
    with torch.no_grad():
        logits, loss = m(sx.cuda(), sy.cuda(), qx.cuda(), qy.cuda())
    feat, keep = m._trace["feat"], m._trace["shot_keep"].cpu().view(2, 5)
    m._trace = None
    from r3dfsseg_amd import ops
    fcm = ops.pm_to_cm(feat, 12, 512).cpu()
    ferr = _close(fcm[:10][:, ::8, ::16], t("support_feat_s"))
    qs = int(g[p + "q_stride"])
    qerr = _close(fcm[10:][:, :, ::qs], t("query_feat_q"))
    ref = t("query_pred")
    rel = (logits.cpu() - ref).abs() / ref.abs().clamp(min=1.0)
    agree = float((logits.cpu().argmax(1) == ref.argmax(1)).float().mean())
    dl = abs(float(loss) - float(g[p + "loss"]))
    print("reference fixture: features (sampled) support %.3e query %.3e; keep %s; logits max %.3e, beyond 1e-4: %.5f; "
          "|loss - ref| %.3e; arg-max agreement %.4f" % (ferr, qerr, keep.tolist(), float(rel.max()),
                                                         float((rel > TOL).float().mean()), dl, agree))
    assert torch.equal(keep.float(), t("clean_flag")), (keep, g[p + "clean_flag"])
    assert float(rel.max()) <= TOL
    assert dl <= TOL * max(1.0, abs(float(g[p + "loss"])))
    assert agree >= 0.99


def test_detection_changes_the_prediction_of_a_noisy_episode():
    """ProtoNet and ProtoNet_Contrast on the same weights differ exactly when a shot is dropped."""
    from r3dfsseg_amd.protonet import ProtoNet
    cfg = S.make_cfg(n_way=2, k_shot=5, n_queries=1, pc_npts=512)
    L = _learner(cfg)
    sd = L.model.state_dict()
    plain = ProtoNet(SimpleNamespace(**cfg)).cuda().eval()
    plain.load_state_dict({k: v for k, v in sd.items() if not k.startswith("proj.")})
    data = [t.cuda() for t in S.make_episode(cfg, 3, noise_ratio=0.4)[0][:4]]
    L.model.eval()
    L.model._trace = {}
    with torch.no_grad():
        a, _ = L.model(*data)
        b, _ = plain(*data)
    assert (L.model._trace["shot_keep"] == 0).any()
    L.model._trace = None
    assert torch.equal(a[:, 0], b[:, 0]) and not torch.equal(a[:, 1:], b[:, 1:])  # background column: every shot, as ever


def test_checkpoint_round_trip(tmp_path):
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    from r3dfsseg_amd.protonet import ProtoNet
    cfg = S.make_cfg(n_way=2, k_shot=5, n_queries=1, pc_npts=512)
    full = S.make_state_dict(cfg, seed=321)
    proto = ProtoNet(SimpleNamespace(**cfg))
    proto.load_state_dict({k: v for k, v in full.items() if not k.startswith("proj.")}, strict=True)
    L = _learner(cfg)
    sd = dict(proto.state_dict())
    sd.update({k: v for k, v in full.items() if k.startswith("proj.")})
    L.model.load_state_dict(sd, strict=True)  # a ProtoNet state dict plus proj.*: strictly
    # ... and a ProtoNet checkpoint file as ProtoLearner saves it (no proj.*) through the learner's own loader
    torch.save(dict(iteration=7, IoU=0.5, model_state_dict=proto.state_dict()), str(tmp_path / "checkpoint.tar"))
    L2 = ProtoContrastLearner(SimpleNamespace(**dict(cfg, model_checkpoint_path=str(tmp_path))), mode='test')
    assert L2.model.checkpoint_meta["missing"] == ["proj.weight", "proj.bias"] and not L2.model.checkpoint_meta["unexpected"]
    got = L2.model.state_dict()
    for k, v in proto.state_dict().items():
        assert torch.equal(got[k].cpu(), v), k
    data = S.make_episode(cfg, 3, noise_ratio=0.4)[0]
    pred, loss, acc = L2.test([t.cuda() for t in data], None)
    L.model.load_state_dict(got, strict=True)
    pred1, loss1, acc1 = L.test([t.cuda() for t in data], None)
    assert torch.equal(pred, pred1) and torch.equal(loss, loss1) and acc == acc1
