"""fit_scene without a device: the argument checks, the entry points' own checks, and the properties of the numpy
restatement (tests/scene_support_ref.py) on the seeded label sets (tests/scene_support_cases.py)."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_cases as SC  # noqa: E402
import scene_support_cases as C  # noqa: E402
from scene_support_ref import RefSupport  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene_support, synthetic as S  # noqa: E402
from r3dfsseg_amd.mpti import MPTI_SelfAtten  # noqa: E402
from r3dfsseg_amd.protonet import ProtoNet, ProtoNet_Contrast  # noqa: E402


def _cpu_model(cls=ProtoNet, **over):
    cfg = S.make_cfg(n_way=2, k_shot=2, pc_npts=64, **over)
    return cls(SimpleNamespace(**cfg)).eval()


@pytest.mark.parametrize("cls", [ProtoNet, ProtoNet_Contrast, MPTI_SelfAtten])
def test_argument_errors_come_before_any_device_work(cls):
    m = _cpu_model(cls)
    scan, labels, classes = torch.zeros(100, 6), torch.zeros(100, dtype=torch.int64), (3, 8)
    for bad in (labels[:99], labels[:, None], labels[None], [0] * 100, None):
        with pytest.raises(ValueError, match=r"labels must be \(M,\)"):
            m.fit_scene(scan, bad, classes)
    for bad in (labels.float(), labels.to(torch.int16), labels.bool(), np.zeros(100, np.uint8)):
        with pytest.raises(ValueError, match="int32 or int64"):
            m.fit_scene(scan, bad, classes)
    for bad in ((3,), (3, 8, 9), (3, 3), (3, 8.0), (3, True), (3, "8"), 5, None):
        with pytest.raises(ValueError, match="classes must be"):
            m.fit_scene(scan, labels, bad)
    for bad in ((3, 2 ** 31), (-2 ** 31 - 1, 3)):
        with pytest.raises(ValueError, match="does not fit in int32"):
            m.fit_scene(scan, labels, bad)
    for bad in (-0.01, 1.0, 1.5, float("nan"), "0.05", None, True):
        with pytest.raises(ValueError, match="min_ratio"):
            m.fit_scene(scan, labels, classes, min_ratio=bad)
    for bad in (-1, 1.5, 10.0, "3", None, True, 2 ** 31):
        with pytest.raises(ValueError, match="min_fg"):
            m.fit_scene(scan, labels, classes, min_fg=bad)
    # everything check_scene_args refuses
    with pytest.raises(ValueError, match="scan must be"):
        m.fit_scene(scan[:, :5], labels, classes)
    with pytest.raises(ValueError, match="float32"):
        m.fit_scene(scan.double(), labels, classes)
    with pytest.raises(ValueError, match="integer in 1..4"):
        m.fit_scene(scan, labels, classes, block_size=1.0, stride=0.4)
    with pytest.raises(ValueError, match="min_points"):
        m.fit_scene(scan, labels, classes, min_points=0)
    m.train()
    with pytest.raises(NotImplementedError):
        m.fit_scene(scan, labels, classes)


def test_accepted_arguments_come_back_as_tensors_and_ints():
    m = _cpu_model()
    scan = np.zeros((50, 6), np.float32)
    for labels, dtype in ((np.zeros(50, np.int32), torch.int32), (torch.zeros(50, dtype=torch.int64), torch.int64)):
        out = scene_support.check_support_args(m, scan, labels, np.array([-2 ** 31, 2 ** 31 - 1]), 1.0, 0.5, 100, 0, np.int64(0))
        assert isinstance(out[0], torch.Tensor) and isinstance(out[1], torch.Tensor) and out[1].dtype == dtype
        assert out[2] == [-2 ** 31, 2 ** 31 - 1] and all(type(c) is int for c in out[2]) and out[3] == 2
    with pytest.raises(ValueError, match=r"way 2 \(class id 8\) has 1 eligible block, k_shot = 2"):
        scene_support.check_eligible([2, 1], [3, 8], 2)
    scene_support.check_eligible([2, 5], [3, 8], 2)


def test_learners_have_fit_scene():
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    from r3dfsseg_amd.proto_learner import ProtoLearner
    for L in (MPTILearner_V3, ProtoLearner, ProtoContrastLearner):
        assert L.fit_scene is F.FittedLearner.fit_scene


def test_entry_points_refuse_null_pointers_and_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    words = lib.r3d_scene_ws_words(1000, 6, 4, 50)
    counts = lambda ws, lab, n, **k: lib.r3d_scene_support_counts(1000, 6, 4, k.get("r", 2), 256, 50, ws, n, lab, k.get("nbytes", 8),
                                                                   p, k.get("n_way", 2), p, None)
    assert counts(None, p, words) != 0 and "null" in err()
    assert counts(p, None, words) != 0 and "null" in err()
    assert counts(p, p, words - 1) != 0 and "workspace" in err()
    assert counts(p, p, words, n_way=8) != 0 and "n_way" in err()
    assert counts(p, p, words, n_way=0) != 0 and "n_way" in err()
    assert counts(p, p, words, nbytes=2) != 0 and "int32 or int64" in err()
    assert counts(p, p, words, r=5) != 0 and "1 .. 4" in err()
    pick = lambda ws, fg, n, **k: lib.r3d_scene_support_pick(1000, 6, 4, 2, 256, 50, ws, n, fg, k.get("n_way", 2), k.get("k_shot", 2),
                                                             k.get("ratio", 0.05), k.get("min_fg", 10), p, p, p, None)
    assert pick(None, p, words) != 0 and "null" in err()
    assert pick(p, None, words) != 0 and "null" in err()
    assert pick(p, p, words - 1) != 0 and "workspace" in err()
    assert pick(p, p, words, n_way=8) != 0 and "n_way" in err()
    assert pick(p, p, words, k_shot=0) != 0 and "k_shot" in err()
    assert pick(p, p, words, ratio=1.0) != 0 and "min_ratio" in err()
    assert pick(p, p, words, ratio=float("nan")) != 0 and "min_ratio" in err()
    assert pick(p, p, words, min_fg=-1) != 0 and "min_fg" in err()
    prep = lambda blocks, out, n, **k: lib.r3d_scene_prepare_blocks(p, 6, 1000, 6, 4, 2, 256, 50, p, n, blocks, k.get("G", 4),
                                                                    k.get("C", 9), 3, 6, out, 9 * 256, 256, 1, None,
                                                                    k.get("lab"), k.get("nbytes", 0), k.get("cls"), k.get("mask"), None)
    assert prep(None, p, words) != 0 and "blocks" in err()
    assert prep(p, None, words) != 0 and "null" in err()
    assert prep(p, p, words - 1) != 0 and "workspace" in err()
    assert prep(p, p, words, G=0) != 0 and "block ids" in err()
    assert prep(p, p, words, G=65537) != 0 and "block ids" in err()
    assert prep(p, p, words, C=6) != 0 and "does not hold" in err()
    assert prep(p, p, words, lab=p, nbytes=8) != 0 and "go together" in err()
    assert prep(p, p, words, lab=p, cls=p, mask=p, nbytes=3) != 0 and "int32 or int64" in err()


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 2])
def test_properties_of_the_restatement(r):
    plan, labels, ref = SC.small_plan(r), C.small_labels(r), C.small_support(r)
    n_way = len(C.CLASSES)
    assert ref.fg.shape == (len(plan.block_list), n_way) and ref.fg.dtype == np.int32
    for b, lst in enumerate(plan.block_list):
        if not plan.kept[b]:
            assert (ref.fg[b] == 0).all() and ref.length[b] == 0
            continue
        members = ref.members[b]
        assert len(set(members)) == len(members) == ref.length[b] <= plan.N and set(members) <= set(lst)
        for w, cls in enumerate(C.CLASSES):  # fg is the class's members of the cloud: each once, none from outside
            assert ref.fg[b, w] == int((labels[members] == cls).sum()) <= int((labels[lst] == cls).sum())
        assert ref.fg[b].sum() <= ref.length[b]
    if r == 1:  # the blocks are disjoint: fg sums to the class's points in all the clouds together
        every = np.array(sorted(p for m in ref.members.values() for p in m))
        assert len(set(every)) == len(every)
        for w, cls in enumerate(C.CLASSES):
            assert int(ref.fg[:, w].sum()) == int((labels[every] == cls).sum())
    for w in range(n_way):  # the order is strict: no two blocks share a key
        keys = [(-int(ref.fg[b, w]), b) for b in ref.eligible[w]]
        assert all(a < b for a, b in zip(keys, keys[1:]))
        assert all(ref.fg[b, w] > ref.thr[b] and plan.kept[b] for b in ref.eligible[w])
        assert all(not plan.kept[b] or ref.fg[b, w] <= ref.thr[b] for b in set(range(len(plan.block_list))) - set(ref.eligible[w]))
    blocks, fgs = ref.pick()
    x, y, sm = ref.shots()
    assert x.shape == (n_way, C.K_SHOT, 9, plan.N) and y.shape == sm.shape == (n_way, C.K_SHOT, plan.N) and y.dtype == np.int32
    assert np.isfinite(x).all() and set(np.unique(y)) <= {0, 1}
    for w in range(n_way):
        assert len(set(blocks[w])) == C.K_SHOT
        for i in range(C.K_SHOT):
            b, ln = blocks[w, i], int(ref.length[blocks[w, i]])
            assert y[w, i].sum() >= fgs[w, i] > 0                      # masks are non-empty
            assert int(y[w, i, :ln].sum()) == fgs[w, i]                  # the first round of slots holds every member once
            assert (sm[w, i] == sm[w, i, np.arange(plan.N) % ln]).all()  # the slots wrap, and the mask with them
            assert (y[w, i] == y[w, i, np.arange(plan.N) % ln]).all()
            assert (sm[w, i, :ln] == np.array(ref.members[b])).all()


@pytest.mark.parametrize("r", [1, 2])
def test_the_short_label_set_raises_in_the_restated_pick(r):
    ref = C.small_support(r, short=True)
    assert ref.n_eligible[1] == C.K_SHOT - 1 and ref.n_eligible[0] >= C.K_SHOT
    with pytest.raises(ValueError, match=r"way 2 \(class id -4\) has 1 eligible"):
        ref.pick()
    with pytest.raises(ValueError):
        ref.shots()


def test_threshold_is_one_fp32_multiplication():
    plan = SC.small_plan(1)
    ref = RefSupport(plan, C.small_labels(1), C.CLASSES, 1, min_ratio=0.3, min_fg=0)
    for b in np.nonzero(plan.kept)[0]:
        assert ref.thr[b] == int(np.floor(np.float32(ref.length[b]) * np.float32(0.3)))
    assert C.as_int32(C.small_labels(1)).dtype == np.int32 and (C.as_int32(C.small_labels(1)) == 7).sum() == (C.small_labels(1) == 7).sum()
