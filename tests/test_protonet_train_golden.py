"""The float64 restatement of the ProtoNet head (tests/protonet_ref.py) against the REFERENCE's own training step
(tests/golden/protonet_train.npz, written by tools/gen_golden_protonet_train.py from models/protonet.py:245-275 under
model.train() with loss.backward(), both dist_methods).  tests/test_gpu_protonet_train.py checks the HIP kernels against this
restatement; here the restatement itself is held to the reference: fed by the oracle's training-mode getFeatures (support
call, then query call, the reference's near-tie kNN rows injected), it reproduces the recorded logits, loss, the gradient
at the two getFeatures results and the BatchNorm running statistics.

Bars: the oracle's features agree with the reference's to 2e-5 absolute (tests/test_oracle_golden_head.py holds that); the
loss is a mean over 1024 points of O(1) terms -> 2e-5; logits 1e-4 (the bar of the MPTI fixtures); the feature gradients are
fp32 autograd results of the reference compared in relative L2 per tensor at the project's feature bar of 1e-4.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from r3dfsseg_amd import _lib, synthetic as S  # noqa: E402
import protonet_ref as R  # noqa: E402
import r3d_oracle as O  # noqa: E402
from test_oracle_golden_head import knn_patches  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "protonet_train.npz")
CFG = dict(n_way=2, k_shot=2, pc_npts=512)
EPISODE = dict(seed=21, noise_ratio=0.34, train=True)


def protonet_train_fixture():
    cfg = S.make_cfg(**CFG)
    sd = {k: torch.as_tensor(v) for k, v in S.make_state_dict(cfg, seed=123).items() if not k.startswith("proj.")}
    data, _ = S.make_episode(cfg, **EPISODE)
    data = [torch.from_numpy(np.ascontiguousarray(d)) if isinstance(d, np.ndarray) else d for d in data]
    return cfg, sd, data, np.load(GOLD)


@pytest.mark.parametrize("method", ["cosine", "euclidean"])
def test_float64_head_on_oracle_features_reproduces_the_reference_step(method):
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    cfg, sd, data, g = protonet_train_fixture()
    n_way, k_shot, N = cfg["n_way"], cfg["k_shot"], cfg["pc_npts"]
    S_ = n_way * k_shot
    sx, sy, qx, qy = data[0].reshape(S_, cfg["pc_in_dim"], N), data[1], data[2], data[3]
    new_stats = {}
    patches = knn_patches(g)
    with torch.no_grad():
        sfeat = O.get_features(sd, sx, cfg, train=True, new_stats=new_stats, idx_override=patches[0])
        qfeat = O.get_features(sd, qx, cfg, train=True, new_stats=new_stats, idx_override=patches[1])
    D = sfeat.shape[1]
    s64 = sfeat.permute(0, 2, 1).reshape(-1, D).double().requires_grad_(True)
    q64 = qfeat.permute(0, 2, 1).reshape(-1, D).double().requires_grad_(True)
    Z = R.head(s64, q64, sy.reshape(S_, N), n_way, k_shot, N, method)
    logits, loss = R.logits_and_loss(Z, qy.to(torch.int64))
    loss.backward()
    pre = method + "/"
    el = float((logits.detach() - torch.from_numpy(g[pre + "logits"]).double()).abs().max())
    dl = abs(float(loss.detach()) - float(g[pre + "loss"]))
    es = R.rel_l2(s64.grad[::8, ::4], torch.from_numpy(g[pre + "dsfeat_s"]))
    eq = R.rel_l2(q64.grad[::8, ::4], torch.from_numpy(g[pre + "dqfeat_s"]))
    print("%s: max |logit - ref| %.2e, |loss - ref| %.2e, dsfeat rel-L2 %.2e, dqfeat rel-L2 %.2e" % (method, el, dl, es, eq))
    assert el <= 1e-4 and dl <= 2e-5
    assert es <= 1e-4 and eq <= 1e-4
    n_buf = 0
    for k, v in new_stats.items():  # running statistics after the support call and the query call
        np.testing.assert_allclose(v.numpy(), g[pre + "buf/" + k], atol=1e-5, rtol=1e-5, err_msg=k)
        n_buf += 1
    assert n_buf == sum(1 for f in g.files if f.startswith(pre + "buf/"))
    assert sum(1 for f in g.files if f.startswith(pre + "gnorm/")) == 35  # every parameter of the reference has a gradient


def test_training_entry_points_are_declared_and_bound():
    names = {"r3d_protonet_head_train_ws_words", "r3d_protonet_head_train_fwd", "r3d_protonet_head_bwd"}
    assert names <= set(_lib._SIGS)
    assert names <= set(_lib.header_symbols())
    assert _lib.ABI_VERSION == 6  # additive change
