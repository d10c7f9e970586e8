"""pool_segments without a device (r3dfsseg_amd/scene_segments.py): the argument checks, the signatures, the ABI, the argument
checks of the new entry points, and the numpy restatement tests/scene_segments_ref.py against hand-written loops."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_segments_ref as R  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene, scene_segments as SS  # noqa: E402

f32 = np.float32


def _res(M=10, C=3, K=0):
    """A SceneResult (K = 0) or SceneSetsResult with host tensors: enough for every check that needs no device."""
    votes = torch.ones(M, dtype=torch.int32)
    labels = torch.zeros(M, dtype=torch.int64)
    if K == 0:
        return scene.SceneResult(labels, torch.zeros(M, C), votes, 1, 1, 0, 0)
    return scene.SceneSetsResult(torch.zeros(M, K, C), torch.zeros(M, K, dtype=torch.int64), votes, labels,
                                 torch.zeros(M, dtype=torch.int32), torch.zeros(M), 1, 1, 0, 0)


def test_argument_errors_are_raised_without_a_device():
    seg = torch.zeros(10, dtype=torch.int64)
    with pytest.raises(ValueError, match="SceneResult or a scene.SceneSetsResult"):
        SS.pool_segments((torch.zeros(10, 3),), seg)
    with pytest.raises(ValueError, match="SceneResult or a scene.SceneSetsResult"):
        SS.pool_segments(None, seg)
    for wrong in (torch.zeros(10, 1, dtype=torch.int64), torch.zeros(10), torch.zeros(10, dtype=torch.int16), [0] * 10,
                  np.zeros(10, np.float32)):
        with pytest.raises(ValueError, match="segments must be an"):
            SS.pool_segments(_res(), wrong)
    with pytest.raises(ValueError, match="9 segment ids for the 10 points"):
        SS.pool_segments(_res(), seg[:9])
    for m in (0, -1, 1.0, True, None, "2"):
        with pytest.raises(ValueError, match="min_members"):
            SS.pool_segments(_res(), seg, min_members=m)
    with pytest.raises(ValueError, match="65 score columns"):
        SS.pool_segments(_res(C=65), seg)
    with pytest.raises(ValueError, match="66 score columns"):
        SS.pool_segments(_res(C=3, K=22), seg)
    # classes and background belong to a sets result
    with pytest.raises(ValueError, match="SceneSetsResult only"):
        SS.pool_segments(_res(), seg, classes=[[1, 2]])
    with pytest.raises(ValueError, match="SceneSetsResult only"):
        SS.pool_segments(_res(), seg, background=0)
    with pytest.raises(ValueError, match="pool_segments: classes must be None or 2 sequences"):
        SS.pool_segments(_res(K=2), seg, classes=[[1, 2]])
    with pytest.raises(ValueError, match="pool_segments: classes"):
        SS.pool_segments(_res(K=2), seg, classes=[[1, 2], [3, 2 ** 31]])
    with pytest.raises(ValueError, match="pool_segments: background"):
        SS.pool_segments(_res(K=2), seg, background=1.5)
    # a result whose fields are not those of its class
    r = _res()
    r.votes = r.votes.to(torch.int64)
    with pytest.raises(ValueError, match="does not hold the tensors"):
        SS.pool_segments(r, seg)
    r = _res(K=2)
    r.set_of = None
    with pytest.raises(ValueError, match="does not hold the tensors"):
        SS.pool_segments(r, seg)
    # everything is in order except the device: said last, still before any launch
    with pytest.raises(ValueError, match="on the device"):
        SS.pool_segments(_res(), seg)
    with pytest.raises(ValueError, match="on the device"):
        SS.pool_segments(_res(K=2), seg.numpy().astype(np.int32), classes=[[1, 2], [3, 4]], background=7)
    # the learners' forward raises the same, and needs no fit
    with pytest.raises(ValueError, match="min_members"):
        F.FittedLearner().pool_segments(_res(), seg, min_members=0)


def test_check_pool_args_returns_what_the_call_needs():
    sets, K, C, seg, table = SS.check_pool_args(_res(), np.arange(10, dtype=np.int32))
    assert (sets, K, C, table) == (False, 0, 3, None) and isinstance(seg, torch.Tensor) and seg.dtype == torch.int32
    sets, K, C, seg, table = SS.check_pool_args(_res(K=3), torch.arange(10), 2, [[5, 6], [6, 7], [8, 9]], 0)
    assert (sets, K, C) == (True, 3, 3) and table.dtype == np.int32 and np.array_equal(table, [[5, 6], [6, 7], [8, 9]])
    assert np.array_equal(SS.check_pool_args(_res(K=2), torch.arange(10))[4], [[0, 1], [2, 3]])
    assert SS.check_pool_args(_res(C=64), torch.arange(10))[2] == 64  # 64 columns are allowed


def test_signatures_and_abi():
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    from r3dfsseg_amd.proto_learner import ProtoLearner
    want = dict(min_members=1, classes=None, background=-1)
    sig = inspect.signature(SS.pool_segments)
    assert list(sig.parameters) == ["res", "segments"] + list(want)
    assert {k: sig.parameters[k].default for k in want} == want
    for L in (MPTILearner_V3, ProtoLearner, ProtoContrastLearner):
        assert L.pool_segments is F.FittedLearner.pool_segments and L.pool_segments.__doc__
        sig = inspect.signature(L.pool_segments)
        assert list(sig.parameters) == ["self", "res", "segments"] + list(want)
        assert {k: sig.parameters[k].default for k in want} == want
    assert _lib.ABI_VERSION == 6
    for name in ("r3d_scene_seg_ws_words", "r3d_scene_seg_ids", "r3d_scene_seg_group", "r3d_scene_seg_pool",
                 "r3d_scene_seg_spread"):
        assert name in _lib.header_symbols()
    # predict_scene and predict_scene_sets are as they were
    assert list(inspect.signature(scene.predict_scene).parameters)[:3] == ["model", "fitted", "scan"]
    assert list(inspect.signature(scene.predict_scene_sets).parameters)[:4] == ["model", "fits", "scan", "classes"]


def test_new_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    M = 1000
    words = lib.r3d_scene_seg_ws_words(M)
    assert words > 9 * M and lib.r3d_scene_seg_ws_words(0) == -1 and lib.r3d_scene_seg_ws_words(2 ** 27 + 1) == -1
    assert lib.r3d_scene_seg_ws_words(2 ** 27) > 0
    ids = lambda seg=p, nbytes=8, M=M, ws=p, w=words: lib.r3d_scene_seg_ids(seg, nbytes, M, ws, w, None)
    assert ids(seg=None) != 0 and "null" in err()
    assert ids(nbytes=2) != 0 and "int32 or int64" in err()
    assert ids(M=0) != 0 and "M 0" in err()
    assert ids(w=words - 1) != 0 and "workspace" in err()
    group = lambda votes=p, max_id=5, n_neg=0, w=words: lib.r3d_scene_seg_group(p, 4, M, votes, max_id, n_neg, p, p, w, None)
    assert group(votes=None) != 0 and "null" in err()
    assert group(max_id=2 ** 31 - 1) != 0 and "largest id" in err()
    assert group(max_id=-2) != 0 and "largest id" in err()
    assert group(n_neg=M + 1) != 0 and "negative ids" in err()
    assert group(w=10) != 0 and "workspace" in err()
    pool = lambda C=3, S=4, T=5, part=p, ids_=p: lib.r3d_scene_seg_pool(M, C, p, p, S, T, p, words, part, ids_, p, p, p, p, None)
    assert pool(C=65) != 0 and "score columns" in err()
    assert pool(S=M + 1) != 0 and "segments" in err()
    assert pool(T=-1) != 0 and "tiles" in err()
    assert pool(part=None) != 0 and "part" in err()
    assert pool(ids_=None) != 0 and "null" in err()
    spread = lambda C=6, K=0, mm=1, sl=None, labels=p: lib.r3d_scene_seg_spread(
        M, C, K, 4, mm, p, p, p, p, sl, sl, sl, p, p, sl, sl, sl, p, labels, p, sl, sl, sl, p, words, None)
    assert spread(labels=None) != 0 and "null" in err()
    assert spread(C=65) != 0 and "score columns" in err()
    assert spread(mm=0) != 0 and "min_members" in err()
    assert spread(K=4) != 0 and "sets over" in err()       # 6 columns are not 4 sets
    assert spread(K=2) != 0 and "with sets" in err()       # the set fields are missing


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _double_loop(rows):
    """P3 written out with scalars: tiles of 256, one float32 addition at a time."""
    n, cols = rows.shape
    tot = [None] * cols
    for j in range(cols):
        t = 0
        while t * 256 < n:
            part = f32(rows[t * 256, j])
            r = t * 256 + 1
            while r < n and r < (t + 1) * 256:
                part = f32(part + rows[r, j])
                r += 1
            tot[j] = part if t == 0 else f32(tot[j] + part)
            t += 1
    return np.array(tot, f32)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_restated_sum_equals_a_hand_written_double_loop(n):
    rs = np.random.RandomState(n)
    rows = (rs.randn(n, 3) * np.array([1.0, 1e4, 1e-3])).astype(f32)
    got = R.pool_rows(rows)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), _double_loop(rows).view(np.uint32))
    # and through pool(): one segment of n contributors with one vote each, scattered among points of no segment
    M = 2 * n + 3
    scores = np.zeros((M, 3), f32)
    scores[1::2][:n] = rows
    segments = np.full(M, -1, np.int64)
    segments[1::2][:n] = 77
    out = R.pool(scores, np.ones(M, np.int32), np.zeros(M, np.int64), segments)
    want = _double_loop(rows) / f32(n)
    assert out["n_segments"] == 1 and out["segment_members"].tolist() == [n] and out["segment_ids"].tolist() == [77]
    assert np.array_equal(out["segment_scores"][0].view(np.uint32), want.view(np.uint32))


def test_the_restatement_is_sensitive_to_the_order():
    """1e8, 1, ..., 1, -1e8, 1 over 257 rows: the 254 ones vanish beside 1e8, -1e8 closes the first tile at 0 and the last
    row is a tile of its own, so P3 gives 1; the exact sum is 255; the same rows in reverse give 0.  A kernel that adds in
    another order cannot match by luck."""
    rows = R.cancelling_rows(257)
    assert rows.shape == (257, 1) and rows[0, 0] == f32(1e8) and rows[255, 0] == f32(-1e8) and (rows[1:255] == 1).all()
    got = R.pool_rows(rows)[0]
    exact = f32(rows.astype(np.float64).sum())
    rev = R.pool_rows(rows[::-1].copy())[0]
    assert exact == f32(255) and got == f32(1) and rev == f32(0)
    assert got != exact and got != rev
    # the tile edge is part of the definition: 1e8 and 511 ones are 1e8 when added in one run, 1e8 + 256 in tiles of 256
    rows = np.ones((512, 1), f32)
    rows[0] = f32(1e8)
    flat = f32(rows[0, 0])
    for v in rows[1:, 0]:
        flat = f32(flat + v)
    assert flat == f32(1e8) and R.pool_rows(rows)[0] == f32(1e8) + f32(256) != flat


def test_untouched_points_keep_the_bits_of_res():
    rs = np.random.RandomState(3)
    M = 40
    scores = rs.randn(M, 3).astype(f32)
    scores[5, 1] = f32(-0.0)
    scores[6, 2] = f32(np.nan)
    votes = rs.randint(0, 4, M).astype(np.int32)
    labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)
    segments = np.full(M, -1, np.int64)
    segments[10:20] = 4          # 10 points
    segments[20:23] = 9          # 3 points, at most 3 members: below min_members = 5
    votes[10:20] = 2
    labels[10:20] = 0
    votes[12] = 0               # a point of segment 4 without a vote: it receives, it does not contribute
    labels[12] = -1
    out = R.pool(scores, votes, labels, segments, min_members=5)
    keep = np.ones(M, bool)
    keep[10:20] = False
    assert not out["pooled"][keep].any() and out["pooled"][10:20].all()
    assert np.array_equal(out["scores"][keep].view(np.uint32), scores[keep].view(np.uint32))
    assert np.array_equal(out["labels"][keep], labels[keep])
    assert out["segment_members"].tolist() == [9, int((votes[20:23] > 0).sum())] and out["segment_points"].tolist() == [10, 3]
    assert (out["scores"][10:20] == out["segment_scores"][0]).all() and (out["labels"][10:20] == out["segment_labels"][0]).all()
    assert out["n_pooled"] == 10 and out["n_filled"] == 1 and out["segment_index"][12] == 0 and out["segment_index"][0] == -1
    # the contributors' rows are scores / votes, the member without a vote is left out of the mean
    rows = np.stack([scores[p] / f32(2) for p in range(10, 20) if p != 12]).astype(f32)
    assert np.array_equal(out["segment_scores"][0], R.pool_rows(rows) / f32(9))
    # with min_members = 1 the small segment pools as well; a segment without a member has no label and a row of zeros
    votes[20:23] = 0
    out = R.pool(scores, votes, labels, segments, min_members=1)
    assert out["segment_members"].tolist() == [9, 0] and out["segment_labels"][1] == -1 and not out["segment_scores"][1].any()
    assert not out["pooled"][20:23].any() and np.array_equal(out["scores"][20:23].view(np.uint32), scores[20:23].view(np.uint32))
