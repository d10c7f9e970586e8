"""ProtoNet_Contrast without a GPU: the model shell and its state-dict names, the refusals, the new entry point's
declaration and binding, and the restatement (tests/protonet_contrast_ref.py) the GPU tests hold the keep head to.

tests/golden/protonet_contrast.npz is written by tools/gen_golden_protonet_contrast.py from the reference's own
ProtoNet_Contrast.  It holds `state_dict_keys` and one episode per shape; the generator's docstring says which conditions
each meets and why."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden", "protonet_contrast.npz")

from r3dfsseg_amd import synthetic as S  # noqa: E402
import protonet_contrast_ref as R  # noqa: E402


def _args(**over):
    return SimpleNamespace(**S.make_cfg(n_way=2, k_shot=5, pc_npts=512, **over))


def test_model_constructs_with_the_reference_state_dict_names():
    from r3dfsseg_amd.protonet import ProtoNet, ProtoNet_Contrast
    m = ProtoNet_Contrast(_args())
    keys = list(m.state_dict().keys())
    assert keys == [str(k) for k in np.load(GOLD)["state_dict_keys"]]
    assert keys == list(ProtoNet(_args()).state_dict().keys()) + ["proj.weight", "proj.bias"]
    assert m.proj.weight.shape == (128, 192)
    m.load_state_dict(S.make_state_dict(S.make_cfg(n_way=2, k_shot=5, pc_npts=512)), strict=True)


def test_feat_dim_other_than_192_is_refused_at_construction():
    from r3dfsseg_amd.protonet import ProtoNet_Contrast
    with pytest.raises(NotImplementedError, match="192"):
        ProtoNet_Contrast(_args(output_dim=32))


def test_training_is_refused():
    from r3dfsseg_amd.protonet import ProtoNet_Contrast
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    m = ProtoNet_Contrast(_args()).eval()
    z = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="evaluation"):
        m(z, z, z, z, train=True)
    with pytest.raises(NotImplementedError, match="evaluation"):
        m.train()(z, z, z, z)
    with pytest.raises(NotImplementedError):
        ProtoContrastLearner(_args(), mode='train')
    with pytest.raises(ValueError):
        ProtoContrastLearner(_args(), mode='validate')


def test_keep_head_is_declared_and_bound():
    from r3dfsseg_amd import _lib
    assert "r3d_protonet_head_keep_batched" in _lib.header_symbols()
    res, args = _lib._SIGS["r3d_protonet_head_keep_batched"]
    plain = _lib._SIGS["r3d_protonet_head_batched"]
    assert res is _lib.c_i and len(args) == len(plain[1]) + 1 == 19
    assert args[:8] == plain[1][:8] and args[8] is _lib.c_f and args[9:] == plain[1][8:]  # shot_keep after support_y


def test_restatement_on_a_case_small_enough_to_do_by_hand():
    # one channel, 2 ways x 2 shots x 2 points; pooled fg = the masked point, bg = the other one (up to the 1e-5)
    sf = torch.tensor([[[[1.0, 10.0]], [[3.0, 20.0]]], [[[5.0, 30.0]], [[7.0, 40.0]]]])
    sy = torch.tensor([[[1, 0], [1, 0]], [[1, 0], [1, 0]]])
    fg, bg = R.masked_pool(sf.double(), sy == 1), R.masked_pool(sf.double(), sy == 0)
    c = 1.0 / (1.0 + 1e-5)
    keep = torch.tensor([[1, 0], [1, 1]])
    p = R.keep_prototypes(fg, bg, keep)[:, 0]
    assert torch.allclose(p, torch.tensor([25.0 * c, 1.0 * c, 6.0 * c], dtype=torch.float64), rtol=1e-12)  # bg: ALL four shots
    p = R.keep_prototypes(fg, bg, None)[:, 0]
    assert torch.allclose(p, torch.tensor([25.0 * c, 2.0 * c, 6.0 * c], dtype=torch.float64), rtol=1e-12)
    with pytest.raises(ValueError):
        R.keep_prototypes(fg, bg, torch.tensor([[0, 0], [1, 1]]))
    z = R.similarity(torch.tensor([[[2.0]]]).double(), torch.tensor([[1.0], [-3.0]]).double(), "euclidean")
    assert torch.allclose(z[0, :, 0], -torch.tensor([(1 + 1e-6) ** 2, (5 + 1e-6) ** 2], dtype=torch.float64))
    z = R.similarity(torch.tensor([[[2.0]]]).double(), torch.tensor([[1.0], [-3.0]]).double(), "cosine")
    assert torch.allclose(z[0, :, 0], torch.tensor([10.0, -10.0], dtype=torch.float64))


@pytest.mark.parametrize("name,n_way,k_shot", [("w2k5", 2, 5), ("w5k2", 5, 2)])
def test_restatement_against_the_reference_episode(name, n_way, k_shot):
    """One episode per shape from the reference's own forward.  (a) a shot is dropped.  gpu_ok = 1 (stored with inputs, used
    on the device): every `cosine_sum > mean` vote is 1e-2 clear -- the continuous reading of (c); the vote fractions and
    flag averages are ratios of small integers, which only a flipped vote can move.  gpu_ok = 0: the episode serves this
    check alone, which runs on the reference's own pooled features and clean_flag and needs no margin.  Then the
    keep-prototype rule against the reference's query_pred at the bar tests/test_oracle_golden_head.py holds the oracle's
    ProtoNet to (atol 2e-5, rtol 1e-5)."""
    g = np.load(GOLD)
    p = name + "/"
    keep = g[p + "clean_flag"]
    assert keep.shape == (n_way, k_shot) and (keep == 0).any() and (keep.sum(1) > 0).all()
    assert int(g[p + "gpu_ok"]) == (1 if name == "w2k5" else 0)
    if int(g[p + "gpu_ok"]):
        assert np.nanmin(np.abs(g[p + "cosine_sum"] - g[p + "cosine_mean"][:, :, None])) >= 1e-2
        assert g[p + "support_x"].shape == (n_way, k_shot, 9, 512)
    # the stored votes give the stored flags: vote > 0.5 per scale, the average over the scales < 0.5 drops, all-dropped resets
    total = (g[p + "vote"] > 0.5).astype(np.float32).mean(1)
    np.testing.assert_array_equal(total, g[p + "total_flag"])
    want_keep = (total >= 0.5).astype(np.float32)
    want_keep[want_keep.sum(1) == 0] = 1.0
    np.testing.assert_array_equal(want_keep, keep)
    protos = R.keep_prototypes(torch.from_numpy(g[p + "pooled_fg"]).double(), torch.from_numpy(g[p + "pooled_bg"]).double(),
                               torch.from_numpy(keep))
    qs = int(g[p + "q_stride"])
    got = R.similarity(torch.from_numpy(g[p + "query_feat_q"]).double(), protos, "cosine")
    assert got.shape[1] == n_way + 1 and got.shape[2] == 512 // qs
    np.testing.assert_allclose(got.numpy(), g[p + "query_pred"][:, :, ::qs], atol=2e-5, rtol=1e-5)
    # and the plain ProtoNet rule does NOT give these numbers: the check can tell the two apart
    plain = R.similarity(torch.from_numpy(g[p + "query_feat_q"]).double(),
                         R.keep_prototypes(torch.from_numpy(g[p + "pooled_fg"]).double(),
                                           torch.from_numpy(g[p + "pooled_bg"]).double(), None), "cosine")
    assert np.abs(plain.numpy() - g[p + "query_pred"][:, :, ::qs]).max() > 1e-3
