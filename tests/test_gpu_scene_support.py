"""fit_scene on the device (r3dfsseg_amd/scene_support.py, csrc/scene.hip) against the numpy restatement
tests/scene_support_ref.py on the seeded label sets of tests/scene_support_cases.py.

Every comparison is torch.equal / np.array_equal: the definition ("Fitting from an annotated scan") fixes
every operation, the counts are integers and the clouds have the bits of r3d_scene_prepare, so no tolerance is used here."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_cases as SC  # noqa: E402
import scene_support_cases as C  # noqa: E402

from r3dfsseg_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu

_plans = {}


def _device_plan(which, r):
    """The device plan of the small or the medium scan at overlap r, built once per session."""
    from r3dfsseg_amd.scene import ScenePlan
    if (which, r) not in _plans:
        scan, cfg = (SC.small_scan()[0], SC.SMALL) if which == "small" else (SC.medium_scan(), SC.MEDIUM)
        _plans[which, r] = ScenePlan(torch.from_numpy(scan).cuda(), cfg["N"], block_size=cfg["stride"] * r, stride=cfg["stride"],
                                     min_points=cfg["min_points"])
    return _plans[which, r]


def _classes_dev():
    return torch.tensor(C.CLASSES, dtype=torch.int32, device="cuda")


def _labels_dev(labels, dtype):
    return torch.from_numpy(labels if dtype == "int64" else C.as_int32(labels)).cuda()


# ---- 1. counts and choice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int64", "int32"])
@pytest.mark.parametrize("which,r", [("small", 1), ("small", 2), ("medium", 2)])
def test_counts_and_choice_equal_the_restatement(which, r, dtype):
    from r3dfsseg_amd import scene_support
    ref = C.small_support(r) if which == "small" else C.medium_support(r)
    d = _device_plan(which, r)
    assert np.array_equal(d.block_points.cpu().numpy(), ref.plan.block_points)
    labels = _labels_dev(ref.labels, dtype)
    assert labels.dtype == getattr(torch, dtype)
    fg, shot_block, shot_fg, rec = scene_support.count_and_pick(d, labels, _classes_dev(), C.K_SHOT, C.MIN_RATIO, C.MIN_FG)
    assert fg.dtype == torch.int32 and torch.equal(fg.cpu(), torch.from_numpy(ref.fg))
    blocks, fgs = ref.pick()
    assert torch.equal(shot_block.cpu(), torch.from_numpy(blocks)) and torch.equal(shot_fg.cpu(), torch.from_numpy(fgs))
    assert rec.tolist() == ref.n_eligible + [0] * (8 - len(ref.n_eligible))
    if which == "medium":
        assert len(ref.plan.block_list) > 256 and max(ref.n_eligible) > 256  # more blocks than the choice has threads


def test_choice_with_more_shots_than_eligible_blocks_and_other_thresholds():
    """k_shot = 5 where way 2 has two eligible blocks: the missing shots are block -1, fg 0; and the fp32 threshold."""
    from r3dfsseg_amd import ops
    from scene_support_ref import RefSupport
    d, ref = _device_plan("small", 2), C.small_support(2)
    fg = torch.from_numpy(ref.fg).cuda()
    blocks, fgs, rec = ops.scene_support_pick(d.M, *d._geometry(), fg, 5, C.MIN_RATIO, C.MIN_FG)
    for w in range(2):
        el = ref.eligible[w][:5]
        assert blocks[w].tolist() == el + [-1] * (5 - len(el))
        assert fgs[w].tolist() == [int(ref.fg[b, w]) for b in el] + [0] * (5 - len(el))
    assert rec.tolist()[:2] == ref.n_eligible
    for ratio, min_fg in ((0.3, 0), (0.0, 0), (0.2345, 3), (0.05, 59), (0.05, 60)):
        other = RefSupport(ref.plan, ref.labels, C.CLASSES, 1, ratio, min_fg)
        blocks, fgs, rec = ops.scene_support_pick(d.M, *d._geometry(), fg, 1, ratio, min_fg)
        assert rec.tolist()[:2] == other.n_eligible and blocks[:, 0].tolist() == [e[0] if e else -1 for e in other.eligible]


# ---- 2. clouds and masks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [2, 1])
def test_prepare_blocks_equals_prepare_on_chunk_0_of_the_blocks(r):
    from r3dfsseg_amd import ops
    d, p = _device_plan("small", r), SC.small_plan(r)
    every = torch.empty(d.n_chunks, 9, 256, device="cuda")
    every_sm = torch.empty(d.n_chunks, 256, device="cuda", dtype=torch.int32)
    d.prepare(0, every, 3, 6, slot_map=every_sm)
    kept = [int(b) for b in np.nonzero(p.kept)[0]]
    dropped = int(np.nonzero(~p.kept)[0][0])
    ids = kept[::-1] + [dropped, -1, len(p.block_list), kept[0]]  # any order, repeats; the three in the middle name no cloud
    blocks = torch.tensor(ids, dtype=torch.int32, device="cuda")
    out = torch.full((len(ids), 9, 256), float("nan"), device="cuda")
    sm = torch.full((len(ids), 256), -7, device="cuda", dtype=torch.int32)
    ops.scene_prepare_blocks(d.scan, *d._geometry(), blocks, out, 3, 6, sm)
    chunk0 = [int(c) for c in p.block_chunk0]
    for g, b in enumerate(ids):
        if 0 <= b < len(p.block_list) and p.kept[b]:
            assert torch.equal(out[g], every[chunk0[b]]) and torch.equal(sm[g], every_sm[chunk0[b]]), (g, b)
        else:
            assert torch.isnan(out[g]).all() and (sm[g] == -7).all(), (g, b)  # left unwritten
    assert np.array_equal(out[0].cpu().numpy(), p.prepared()[p.block_chunk0[kept[-1]]])


@pytest.mark.parametrize("dtype", ["int64", "int32"])
@pytest.mark.parametrize("r", [2, 1])
def test_clouds_masks_and_slots_equal_the_restatement_in_both_layouts(r, dtype):
    from r3dfsseg_amd import ops, scene_support
    from r3dfsseg_amd.scene import staging
    d, ref = _device_plan("small", r), C.small_support(r)
    x, y, sm = (torch.from_numpy(a) for a in ref.shots())
    labels = _labels_dev(ref.labels, dtype)
    shot_block = torch.from_numpy(ref.pick()[0]).cuda()
    sx, sy, smap = scene_support.prepare_shots(d, shot_block, labels, _classes_dev(), 9, 3, 6)
    assert sx.is_contiguous() and sx.shape == (2, 2, 9, 256) and sy.dtype == smap.dtype == torch.int32
    assert torch.equal(sx.cpu(), x) and torch.equal(sy.cpu(), y) and torch.equal(smap.cpu(), sm)
    assert (sy.sum(-1) > 0).all() and not torch.isnan(sx).any()
    pm = staging(4, 9, 256, "cuda")  # point-major rows, viewed (S, C, N)
    assert ops.is_point_major_view(pm) and not pm.is_contiguous()
    pm.transpose(1, 2).fill_(float("nan"))
    px, py, pmap = scene_support.prepare_shots(d, shot_block, labels, _classes_dev(), 9, 3, 6, out=pm)
    assert px.data_ptr() == pm.data_ptr() and torch.equal(px, sx) and torch.equal(py, sy) and torch.equal(pmap, smap)


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
# name -> (learner, cfg overrides, eval flag of the fit): n_way, k_shot and pc_npts are those of the label sets
CASES = {
    "proto": ("proto_learner.ProtoLearner", dict(dist_method="cosine"), False),
    "contrast": ("proto_contrast_learner.ProtoContrastLearner", dict(), False),
    "mpti": ("mpti_learner.MPTILearner_V3", dict(n_subprototypes=20), True),
}
_learners = {}
SCENE_KW = dict(stride=0.5, min_points=100, min_ratio=C.MIN_RATIO, min_fg=C.MIN_FG)


def _learner(name):
    if name not in _learners:
        import importlib
        path, over, ev = CASES[name]
        mod, cls = path.split(".")
        cfg = S.make_cfg(n_way=2, k_shot=C.K_SHOT, pc_npts=SC.SMALL["N"], **over)
        learner = getattr(importlib.import_module("r3dfsseg_amd." + mod), cls)(
            SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
        _learners[name] = (learner, cfg, ev)
    return _learners[name]


def _logits(learner, q):
    with torch.no_grad():
        return learner.model.predict(learner.fitted, q)[0]


@pytest.mark.parametrize("name", list(CASES))
def test_fit_scene_equals_fit_on_the_restated_support_set(name):
    learner, cfg, ev = _learner(name)
    r = 2
    scan, ref = SC.small_scan()[0], C.small_support(r)
    x, y, sm = (torch.from_numpy(a) for a in ref.shots())
    blocks, fgs = ref.pick()
    q = S.make_episode(cfg, seed=3)[0][2].cuda()
    sup = learner.fit_scene(scan, ref.labels, C.CLASSES, block_size=0.5 * r, eval=ev, **SCENE_KW)  # numpy, int64, from the host
    assert learner.fitted is sup.fitted and sup.n_eligible == ref.n_eligible
    assert torch.equal(sup.shot_block.cpu(), torch.from_numpy(blocks)) and torch.equal(sup.shot_fg.cpu(), torch.from_numpy(fgs))
    assert torch.equal(sup.support_x.cpu(), x) and torch.equal(sup.support_y.cpu(), y) and torch.equal(sup.slot_map.cpu(), sm)
    z_scene = _logits(learner, q)
    assert z_scene.shape == (q.shape[0], 3, 256) and torch.isfinite(z_scene).all()
    # two calls give the same bits; the second takes int32 labels that are already on the device
    again = learner.fit_scene(torch.from_numpy(scan).cuda(), torch.from_numpy(C.as_int32(ref.labels)).cuda(), list(C.CLASSES),
                              block_size=0.5 * r, eval=ev, **SCENE_KW)
    assert again.fitted is not sup.fitted and learner.fitted is again.fitted
    for a, b in ((again.support_x, sup.support_x), (again.support_y, sup.support_y), (again.slot_map, sup.slot_map),
                 (again.shot_block, sup.shot_block), (again.shot_fg, sup.shot_fg)):
        assert torch.equal(a, b)
    assert torch.equal(_logits(learner, q), z_scene)
    res = learner.predict_scene(scan, block_size=0.5 * r, stride=0.5, min_points=100)
    assert res.labels.shape == (scan.shape[0],) and res.n_chunks == SC.small_plan(r).n_chunks and int((res.labels >= 0).sum()) > 0
    # the short label set: ValueError, and the latest fit stays
    short = C.small_labels(r, short=True)
    with pytest.raises(ValueError, match=r"way 2 \(class id -4\) has 1 eligible block, k_shot = 2"):
        learner.fit_scene(scan, short, C.CLASSES, block_size=0.5 * r, eval=ev, **SCENE_KW)
    assert learner.fitted is again.fitted
    # fit() on the restated clouds and masks: the same logits
    learner.fit((x, y), eval=ev)
    assert learner.fitted is not again.fitted
    z_fit = _logits(learner, q)
    assert torch.equal(z_scene, z_fit), (name, (z_scene - z_fit).abs().max().item())


def test_fit_scene_at_r_1_on_a_model_without_colour():
    """r = 1 through the learner; and an xyzXYZ model, whose scan has three columns."""
    learner, cfg, ev = _learner("proto")
    scan, ref = SC.small_scan()[0], C.small_support(1)
    x, y, sm = (torch.from_numpy(a) for a in ref.shots())
    sup = learner.fit_scene(scan, ref.labels, C.CLASSES, block_size=0.5, **SCENE_KW)
    assert torch.equal(sup.support_x.cpu(), x) and torch.equal(sup.support_y.cpu(), y) and torch.equal(sup.slot_map.cpu(), sm)
    from r3dfsseg_amd.proto_learner import ProtoLearner
    cfg3 = S.make_cfg(n_way=2, k_shot=C.K_SHOT, pc_npts=256, pc_in_dim=6, pc_attribs="xyzXYZ", dist_method="cosine")
    plain = ProtoLearner(SimpleNamespace(**dict(cfg3, model_checkpoint_path="synthetic")), mode="test")
    sup3 = plain.fit_scene(np.ascontiguousarray(scan[:, :3]), ref.labels, C.CLASSES, block_size=0.5, **SCENE_KW)
    x3 = torch.from_numpy(ref.shots(rgb=False, XYZ=True)[0])
    assert torch.equal(sup3.support_x.cpu(), x3) and torch.equal(sup3.support_y.cpu(), y) and plain.fitted is sup3.fitted
