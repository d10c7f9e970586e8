"""Host side of predict_scene's cap on the chunks of a block and of the transfer (r3dfsseg_amd/scene.py): the new arguments
are refused with no device present, every learner and model takes them, and the numpy restatement the GPU tests compare
with (tests/scene_sparse_ref.py) has the properties the definition promises."""
import ctypes
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_cases as SC  # noqa: E402
import scene_sparse_ref as SR  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene, synthetic as S  # noqa: E402
from r3dfsseg_amd.mpti import MPTI_SelfAtten  # noqa: E402
from r3dfsseg_amd.protonet import ProtoNet, ProtoNet_Contrast  # noqa: E402


def _cpu_model(cls):
    m = cls(SimpleNamespace(**S.make_cfg(n_way=2, k_shot=1, pc_npts=64)))
    return m.eval()


@pytest.mark.parametrize("cls", [ProtoNet, ProtoNet_Contrast, MPTI_SelfAtten])
def test_new_arguments_are_refused_before_any_device_work(cls):
    m = _cpu_model(cls)
    f = F.FittedSupport(m, protos=torch.zeros(1, 3, m.feat_dim))
    scan = torch.zeros(100, 6)
    for bad in (0, 1.5, "2", -1, True):
        with pytest.raises(ValueError, match="max_chunks_per_block"):
            m.predict_scene(f, scan, max_chunks_per_block=bad)
    for bad in ("linear", "Nearest", 1):
        with pytest.raises(ValueError, match="transfer"):
            m.predict_scene(f, scan, transfer=bad)
    with pytest.raises(ValueError, match="min_points"):  # the earlier checks still come first
        m.predict_scene(f, scan, min_points=0, max_chunks_per_block=0)
    assert scene.check_scene_args(m, scan, 1.0, None, 100, 32, 3, "nearest")[1] == 1
    assert scene.check_scene_args(m, scan, 1.0, None, 100, 32, np.int64(1), None)[1] == 1


def test_learners_and_models_accept_the_keywords():
    from r3dfsseg_amd.dgcnn import FewShotFeatures
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    from r3dfsseg_amd.proto_learner import ProtoLearner
    learner = ["self", "scan", "block_size", "stride", "min_points", "groups_per_launch", "fitted", "max_chunks_per_block",
               "transfer"]
    for L in (MPTILearner_V3, ProtoLearner, ProtoContrastLearner, F.FittedLearner):
        sig = inspect.signature(L.predict_scene)
        assert list(sig.parameters) == learner
        assert sig.parameters["max_chunks_per_block"].default is None and sig.parameters["transfer"].default is None
    model = ["self", "fitted", "scan", "block_size", "stride", "min_points", "groups_per_launch", "launch",
             "max_chunks_per_block", "transfer"]
    assert list(inspect.signature(FewShotFeatures.predict_scene).parameters) == model
    assert list(inspect.signature(scene.predict_scene).parameters) == ["model"] + model[1:]
    with pytest.raises(ValueError, match="call fit"):
        F.FittedLearner().predict_scene(torch.zeros(10, 6), max_chunks_per_block=1, transfer="nearest")
    # the result keeps its constructor and gains keyword attributes with defaults
    res = scene.SceneResult(1, 2, 3, 4, 5, 6, 7)
    assert (res.labels, res.scores, res.votes, res.n_blocks, res.n_chunks, res.n_unlabelled, res.redone) == (1, 2, 3, 4, 5, 6, 7)
    assert res.source is None and res.n_transferred == 0 and res.n_chunks_skipped == 0


@pytest.mark.parametrize("r", [1, 2])
def test_a_cap_that_skips_nothing_is_the_plan(r):
    p = SC.small_plan(r)
    nc_max = int(np.diff(p.block_chunk0).max())
    logits = SR.random_logits(p.n_chunks, p.N, 3)
    want = p.vote(logits)
    for cap in (None, nc_max, nc_max + 5):
        run = SR.RunPlan(p, cap)
        assert run.n_run == p.n_chunks and run.n_skipped == 0
        assert np.array_equal(run.run_chunk0, p.block_chunk0) and np.array_equal(run.run_block, p.chunk_block)
        assert np.array_equal(run.slot_map, p.slot_map)
        for a, b in zip(run.vote(logits), want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    short = SR.RunPlan(p, nc_max - 1)
    assert short.n_skipped == int((np.diff(p.block_chunk0) == nc_max).sum()) > 0


def _transfer_over_all_voted_points(p, votes):
    """Step 9 the long way: every voted point of the scan is looked at, and kept when its cell is within one of the
    receiver's in x and in y."""
    source = np.where(votes > 0, np.arange(p.M), -1).astype(np.int64)
    voted = np.nonzero(votes > 0)[0]
    cx, cy = p.key % p.ncx, p.key // p.ncx
    for rcv in np.nonzero(p.valid & (votes == 0))[0]:
        near = voted[(np.abs(cx[voted] - cx[rcv]) <= 1) & (np.abs(cy[voted] - cy[rcv]) <= 1)]
        if len(near):
            source[rcv] = SR.nearest(p.scan, near, rcv)
    return source


@pytest.mark.parametrize("name", ["small r=1 c=1", "small r=2 c=1", "small r=2 c=2"])
def test_properties_of_the_restated_transfer(name):
    c = SR.case(name)
    p, votes, source = c.p, c.votes, c.source
    M = p.M
    assert int(votes.sum()) == c.run.n_run * p.N and c.run.n_run + c.run.n_skipped == p.n_chunks
    # source[p] == p exactly for the voted points; invalid points have none
    assert np.array_equal(source == np.arange(M), votes > 0) and (source[~p.valid] == -1).all()
    got = (votes == 0) & (source >= 0)
    assert c.n_transferred == int(got.sum()) > 0 and (votes[source[got]] > 0).all()
    # a transferred point's scores and label are its source's; every other point is as the vote left it
    assert np.array_equal(c.t_scores[got], c.scores[source[got]]) and np.array_equal(c.t_labels[got], c.labels[source[got]])
    assert np.array_equal(c.t_scores[~got], c.scores[~got]) and np.array_equal(c.t_labels[~got], c.labels[~got])
    assert (c.t_labels[got] >= 0).all() and c.n_unlabelled == M - int((votes > 0).sum()) - c.n_transferred
    # the cell-restricted search equals a search over all voted points filtered by cell distance
    assert np.array_equal(source, _transfer_over_all_voted_points(p, votes))
    # and the per-cell vectorised form equals the loop
    by_cell = SR.transfer_by_cell(p, c.scores, c.labels, votes)
    for a, b in zip(by_cell, (c.t_scores, c.t_labels, source, c.n_transferred)):
        assert np.array_equal(a, b)
    # the winner is no farther than any other candidate
    for rcv in np.nonzero(got)[0][:50]:
        cand = np.concatenate([[q for q in p.cells[k] if votes[q] > 0] for k in SR.neighbour_cells(p, int(p.key[rcv]))]).astype(int)
        d = SR.distance(p.scan, cand, rcv)
        dq = SR.distance(p.scan, np.array([source[rcv]]), rcv)[0]
        assert dq == d.min() and source[rcv] == cand[d == dq].min()


def test_distance_is_fp32_and_infinity_is_a_value():
    scan = np.array([[0, 0, 0], [3e19, 0, 0], [-3e19, 1, 0], [1, 2, 2]], np.float32)
    d = SR.distance(scan, np.array([1, 2, 3]), 0)
    assert d.dtype == np.float32 and np.isinf(d[0]) and np.isinf(d[1]) and d[2] == 9.0
    assert SR.nearest(scan, np.array([1, 2]), 0) == 1  # two candidates at +inf: the lower index


def test_new_entry_points_refuse_null_pointers_and_short_workspaces():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    assert _lib.ABI_VERSION == 6
    words, sw = lib.r3d_scene_ws_words(1000, 6, 4, 50), lib.r3d_scene_sparse_ws_words(1000, 6, 4, 50)
    assert sw > 5 * 1000 and lib.r3d_scene_sparse_ws_words(1000, 300, 300, 50) == -1
    offs = (ctypes.c_long * 8)()
    assert lib.r3d_scene_sparse_ws_offsets(1000, 6, 4, 50, offs) == 0
    o = list(offs)
    assert len(set(o)) == 8 and all(0 <= v < sw and v % 4 == 0 for v in o) and o[5] + 4 * 1000 == sw
    assert lib.r3d_scene_sparse_ws_offsets(1000, 6, 4, 50, None) != 0
    run = lambda ws, sws, n, sn, cap=2: lib.r3d_scene_run_tables(1000, 6, 4, 2, 256, 50, ws, n, cap, sws, sn, None)
    assert run(None, p, words, sw) != 0 and "null" in err()
    assert run(p, None, words, sw) != 0 and "null" in err()
    assert run(p, p, words - 1, sw) != 0 and "workspace" in err()
    assert run(p, p, words, sw - 1) != 0 and "sparse workspace" in err()
    assert run(p, p, words, sw, cap=0) != 0 and "max_chunks" in err()
    prep = lambda sws, sn: lib.r3d_scene_prepare(p, 6, 1000, 6, 4, 2, 256, 50, p, words, sws, sn, 0, 8, 9, 3, 6, p, 9 * 256, 1, 9,
                                                 None, None)
    assert prep(None, sw) != 0 and "null" in err()
    assert prep(p, sw - 1) != 0 and "sparse workspace" in err()
    vote = lambda sws, sn: lib.r3d_scene_vote(1000, 6, 4, 2, 256, 50, p, words, sws, sn, p, 10, 3, p, p, p, None)
    assert vote(None, sw) != 0 and "null" in err()
    assert vote(p, sw - 1) != 0 and "sparse workspace" in err()
    tr = lambda src, n, sn, K=3: lib.r3d_scene_transfer(p, 6, 1000, 6, 4, 50, p, n, p, sn, K, p, p, p, src, None, None, None)
    assert tr(None, words, sw) != 0 and "null" in err()
    assert tr(p, words - 1, sw) != 0 and "workspace" in err()
    assert tr(p, words, sw - 1) != 0 and "sparse workspace" in err()
    assert tr(p, words, sw, K=65) != 0 and "n_classes" in err()


def test_optional_arguments_are_both_there_or_both_absent():
    """ABI 6: sws of r3d_scene_prepare / r3d_scene_vote is NULL with 0 words (no cap) or a whole sparse workspace; neighbours
    and weights of r3d_scene_transfer come together ("idw") or not at all ("nearest").  The NULL / 0 form gets past those
    checks: the call then fails on a later one, a short ws."""
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    words, sw = lib.r3d_scene_ws_words(1000, 6, 4, 50), lib.r3d_scene_sparse_ws_words(1000, 6, 4, 50)
    prep = lambda sws, sn, n=words: lib.r3d_scene_prepare(p, 6, 1000, 6, 4, 2, 256, 50, p, n, sws, sn, 0, 8, 9, 3, 6, p, 9 * 256, 1,
                                                          9, None, None)
    vote = lambda sws, sn, n=words: lib.r3d_scene_vote(1000, 6, 4, 2, 256, 50, p, n, sws, sn, p, 10, 3, p, p, p, None)
    for call in (prep, vote):
        assert call(None, sw) != 0 and "null" in err()
        assert call(None, 1) != 0 and "null" in err()
        assert call(None, 0, words - 1) != 0 and "null" not in err() and "sparse" not in err() and "workspace" in err()
        assert call(p, sw, words - 1) != 0 and "null" not in err() and "sparse" not in err() and "workspace" in err()
    tr = lambda nbr, wgt, n=words: lib.r3d_scene_transfer(p, 6, 1000, 6, 4, 50, p, n, p, sw, 3, p, p, p, p, nbr, wgt, None)
    assert tr(p, None) != 0 and "null" in err()
    assert tr(None, p) != 0 and "null" in err()
    for both in (None, p):
        assert tr(both, both, words - 1) != 0 and "null" not in err() and "workspace" in err()
