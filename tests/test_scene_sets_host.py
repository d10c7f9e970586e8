"""Host side of predict_scene_sets (r3dfsseg_amd/scene.py, fitted.py): every argument error is raised with no device
present, the numpy restatement of the merge (tests/scene_sets_ref.py) has the properties the definition promises, and
predict_scene keeps its signatures."""
import ctypes
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_sets_ref as R  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene, synthetic as S  # noqa: E402
from r3dfsseg_amd.mpti import MPTI_SelfAtten  # noqa: E402
from r3dfsseg_amd.protonet import ProtoNet, ProtoNet_Contrast  # noqa: E402

f32 = np.float32


def _cpu_model(cls, **over):
    m = cls(SimpleNamespace(**S.make_cfg(**dict(dict(n_way=2, k_shot=1, pc_npts=64), **over))))
    return m.eval()


def _fit(m, **kw):
    """A fit of the model's own kind, with no device: the tables are never read by the checks."""
    if m.fit_table == "head":
        return F.FittedSupport(m, head=F.FittedHead(None, None, 0, None, None, 0), **kw)
    return F.FittedSupport(m, protos=torch.zeros(1, m.n_way + 1, m.feat_dim), **kw)


@pytest.mark.parametrize("cls", [ProtoNet, ProtoNet_Contrast, MPTI_SelfAtten])
def test_arguments_are_refused_before_any_device_work(cls):
    m = _cpu_model(cls)
    scan = torch.zeros(100, 6)
    fits = [_fit(m), _fit(m), _fit(m)]
    call = lambda fits=fits, scan=scan, **kw: m.predict_scene_sets(fits, scan, **kw)
    # fits
    for bad in (None, fits[0], (), [], iter(fits)):
        with pytest.raises(ValueError, match="fits"):
            call(bad)
    with pytest.raises(ValueError, match=r"fits\[1\].*fit_support returned"):
        call([fits[0], "fit"])
    with pytest.raises(ValueError, match="at most 64"):
        call([fits[0]] * 22)  # 22 * 3 = 66 columns
    assert len(F.check_sets_args(m, [fits[0]] * 21)) == 21
    other = _cpu_model(cls)
    with pytest.raises(ValueError, match=r"fits\[2\].*another model"):
        call([fits[0], fits[1], _fit(other)])
    with pytest.raises(ValueError, match=r"fits\[1\].*schedule"):
        call([fits[0], _fit(m, schedule="conservative")])
    wrong = F.FittedSupport(m, protos=None, head=None)
    with pytest.raises(ValueError, match=r"fits\[0\] holds no"):
        call([wrong])
    shape = _fit(m)
    shape.shape = (3, 1, 9, 64)
    with pytest.raises(ValueError, match=r"fits\[0\].*episode shape"):
        call([shape])
    # classes and background
    for bad in ([[0, 1]], [[0, 1], [2, 3], [4]], [[0, 1], [2, 3], [4, 5.0]], [[0, 1], [2, 3], [4, 2 ** 31]], "abc", 7,
                [[0, 1], [2, 3], [4, True]], [0, 1, 2]):
        with pytest.raises(ValueError, match="classes"):
            call(classes=bad)
    for bad in (1.0, None, "0", True, 2 ** 63):
        with pytest.raises(ValueError, match="background"):
            call(background=bad)
    # what predict_scene refuses about the scan and the block arguments is refused here as well
    with pytest.raises(ValueError, match="scan must be"):
        call(scan=torch.zeros(100, 5))
    with pytest.raises(ValueError, match="min_points"):
        call(min_points=0)
    with pytest.raises(ValueError, match="groups_per_launch"):
        call(groups_per_launch=0)
    with pytest.raises(ValueError, match="block_size / stride"):
        call(block_size=1.0, stride=0.3)
    with pytest.raises(ValueError, match="max_chunks_per_block"):
        call(max_chunks_per_block=0)
    with pytest.raises(ValueError, match="transfer"):
        call(transfer="linear")
    # a stale fit: ONE reading of the model's key serves every fit
    with torch.no_grad():
        next(m.parameters()).add_(1e-3)
    with pytest.raises(ValueError, match=r"fits\[0\].*stale fit"):
        call()
    m.train()
    with pytest.raises(NotImplementedError):
        call()


def test_one_key_reading_for_all_fits(monkeypatch):
    m = _cpu_model(ProtoNet)
    fits = [_fit(m) for _ in range(5)]
    calls = []
    real = F.content_sum
    monkeypatch.setattr(F, "content_sum", lambda mod: calls.append(1) or real(mod))
    sets = F.check_sets_args(m, fits)
    assert isinstance(sets, F.FittedSets) and len(sets) == 5 and sets.table is None and len(calls) == 1
    assert all(a is b for a, b in zip(sets, fits))


def test_class_table():
    assert np.array_equal(scene.check_sets_classes(3, 2, None, -1), [[0, 1], [2, 3], [4, 5]])
    t = scene.check_sets_classes(2, 2, [(7, 7), np.array([-2 ** 31, 2 ** 31 - 1])], np.int64(-5))
    assert t.dtype == np.int32 and np.array_equal(t, [[7, 7], [-2 ** 31, 2 ** 31 - 1]])  # the same id in several sets is fine
    assert scene.check_sets_classes(1, 1, [[3]], -2 ** 63).shape == (1, 1)


def test_signatures():
    from r3dfsseg_amd.dgcnn import FewShotFeatures
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    from r3dfsseg_amd.proto_learner import ProtoLearner
    # predict_scene is as it was
    learner = ["self", "scan", "block_size", "stride", "min_points", "groups_per_launch", "fitted", "max_chunks_per_block",
               "transfer"]
    model = ["self", "fitted", "scan", "block_size", "stride", "min_points", "groups_per_launch", "launch",
             "max_chunks_per_block", "transfer"]
    for L in (MPTILearner_V3, ProtoLearner, ProtoContrastLearner, F.FittedLearner):
        assert list(inspect.signature(L.predict_scene).parameters) == learner
    assert list(inspect.signature(FewShotFeatures.predict_scene).parameters) == model
    assert list(inspect.signature(scene.predict_scene).parameters) == ["model"] + model[1:]
    assert list(inspect.signature(scene.SceneResult.__init__).parameters)[1:8] == [
        "labels", "scores", "votes", "n_blocks", "n_chunks", "n_unlabelled", "redone"]
    # the new method
    want = dict(classes=None, block_size=1.0, stride=None, min_points=100, groups_per_launch=32, max_chunks_per_block=None,
                transfer=None, background=-1)
    for L in (MPTILearner_V3, ProtoLearner, ProtoContrastLearner, F.FittedLearner):
        sig = inspect.signature(L.predict_scene_sets)
        assert list(sig.parameters) == ["self", "scan", "fits"] + list(want)
        assert {k: sig.parameters[k].default for k in want} == want
    sig = inspect.signature(FewShotFeatures.predict_scene_sets)
    assert list(sig.parameters)[:3] == ["self", "fits", "scan"] and sig.parameters["launch"].default is None
    assert list(inspect.signature(scene.predict_scene_sets).parameters) == ["model"] + list(sig.parameters)[1:]
    assert _lib.ABI_VERSION == 6
    for name in ("r3d_scene_merge_sets", "r3d_protonet_similarity_sets", "r3d_head_attach_queries_sets"):
        assert name in _lib.header_symbols()


def test_new_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    merge = lambda K=3, C=3, M=10, scores=p, classes=p: lib.r3d_scene_merge_sets(M, K, C, scores, p, None, classes, -1, p, p, p, p,
                                                                                 None)
    assert merge(scores=None) != 0 and "null" in err()
    assert merge(classes=None) != 0 and "null" in err()
    assert merge(K=22) != 0 and "64 score columns" in err()
    assert merge(C=1) != 0 and "at least 2" in err()
    assert merge(M=0) != 0 and "M 0" in err()
    sim = lambda G=2, K=3, n_way=2, q=p: lib.r3d_protonet_similarity_sets(G, K, q, 192, 64, 192, p, 3 * 192, n_way, 64, 0, 10.0, p,
                                                                          None)
    assert sim(q=None) != 0 and "null" in err()
    assert sim(K=22) != 0 and "64 prototype rows" in err()
    assert sim(G=0) != 0 and "groups" in err()
    att = lambda G=3, K=2, fits=p, n_cap=200: lib.r3d_head_attach_queries_sets(G, K, fits, 192, 200, 63, p, 192, 64, 2, 192, 64, p,
                                                                                192, n_cap, p, p, 32, p, 200, None)
    assert att(fits=None) != 0 and "null" in err()
    assert att(n_cap=100) != 0 and "n_cap" in err()
    assert att(G=40000) != 0 and "65535" in err()


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _one(rows, **kw):
    """merge() of one point with a vote: rows = the K score rows."""
    sl, lab, so, mg = R.merge(np.array([rows], f32), np.array([1], np.int32), **kw)
    return sl[0].tolist(), int(lab[0]), int(so[0]), mg[0]


def test_restated_merge_on_hand_made_rows():
    assert R.argmax_lowest(np.array([1, 3, 3], f32)) == (1, 3) and R.argmax_lowest(np.array([1, 3, 3], f32), skip=1) == (2, 3)
    assert R.argmax_lowest(np.array([np.nan, 5], f32))[0] == 0 and R.argmax_lowest(np.array([5, np.nan], f32))[0] == 0
    # the greatest margin wins; classes map (set, way) to an id
    assert _one([[0, 2, 1], [0, 1, 4]]) == ([1, 2], 3, 1, f32(3))
    assert _one([[0, 2, 1], [0, 1, 4]], classes=[[10, 11], [12, 10]]) == ([1, 2], 10, 1, f32(3))
    # equal margins: the lowest set
    assert _one([[0, 1, 2.5], [0, 2.5, 1]]) == ([2, 1], 1, 0, f32(1.5))
    # a tie with class 0 is background; ties between foreground classes take the lowest, with margin 0 -- still a claim
    assert _one([[1, 1, 0], [0, -1, -1]], background=99) == ([0, 0], 99, -1, f32(0))
    assert _one([[0, 2, 2], [3, 0, 0]]) == ([1, 0], 0, 0, f32(0))
    # the margin is against the runner-up, not against class 0
    assert _one([[-5, 3, 2.75]]) == ([1], 0, 0, f32(0.25))
    # +inf is a value; inf - inf is NaN and does not claim
    assert _one([[0, np.inf, 1], [0, 1, 50]]) == ([1, 2], 0, 0, f32(np.inf))
    assert _one([[0, np.inf, np.inf], [0, 1, 1.5]]) == ([1, 2], 3, 1, f32(0.5))
    assert _one([[0, np.inf, np.inf]], background=-7) == ([1], -7, -1, f32(0))
    # fp32: one rounded subtraction
    a, b = f32(16777216.0), f32(0.1)
    assert _one([[b, a]])[3] == f32(a - b) == a
    # without a label: nothing, whatever the scores and the background say
    sl, lab, so, mg = R.merge(np.array([[[0, 9]], [[0, 9]], [[0, 9]]], f32), np.array([0, 0, 0], np.int32),
                              source=np.array([-1, 2, 0]), background=5)
    assert sl[:, 0].tolist() == [-1, 1, 1] and lab.tolist() == [-1, 0, 0] and so.tolist() == [-1, 0, 0] and mg.tolist() == [0, 9, 9]
    assert R.merge(np.zeros((2, 1, 2), f32), np.array([0, 1], np.int32))[1].tolist() == [-1, -1]  # background -1 looks like no label


@pytest.mark.parametrize("K,C", [(1, 2), (3, 3), (8, 8)])
def test_restated_merge_properties(K, C):
    sc, votes, source = R.crafted(K, C, 301, seed=K)
    cls = R.default_classes(K, C - 1)
    sl, lab, so, mg = R.merge(sc, votes, source, background=-3)
    has = (votes > 0) | (source >= 0)
    assert (~has).sum() >= 10 and ((votes == 0) & has).sum() >= 10
    assert (sl[~has] == -1).all() and (lab[~has] == -1).all() and (so[~has] == -1).all() and (mg[~has] == 0).all()
    assert (sl[has] >= 0).all() and (sl[has] < C).all()
    claimed = so >= 0
    assert claimed[has].any() and (~claimed[has]).any() and (lab[has & ~claimed] == -3).all() and (mg[~claimed] == 0).all()
    p = np.nonzero(claimed)[0]
    assert np.array_equal(lab[p], cls[so[p], sl[p, so[p]] - 1]) and (sl[p, so[p]] >= 1).all() and (mg[p] >= 0).all()
    clean = has & np.isfinite(sc).all((1, 2))
    # on finite rows: set_labels is numpy's arg-max (first maximum), and a point is claimed exactly when a set says foreground
    assert np.array_equal(sl[clean], sc[clean].argmax(2)) and np.array_equal(claimed[clean], (sl[clean] >= 1).any(1))
    with np.errstate(invalid="ignore"):
        top2 = np.sort(sc, 2)[:, :, -2:]
        m_all = np.where(sl >= 1, top2[:, :, 1] - top2[:, :, 0], f32(-1))
    assert np.array_equal(mg[clean & claimed], m_all[clean & claimed].max(1))
    assert np.array_equal(so[clean & claimed], m_all[clean & claimed].argmax(1))  # the first set with the greatest margin
    assert so[0] == 0 and mg[0] == 1.5 and so[1] == K - 1       # equal margins: lowest set; the greatest margin wins
    assert so[2] == -1 and so[4] == -1                          # a tie with class 0 does not claim; all background
    assert np.isinf(mg[5]) and so[5] == K - 1
