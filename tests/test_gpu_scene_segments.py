"""pool_segments on the device (r3dfsseg_amd/scene_segments.py, csrc/scene_segments.hip) against the numpy restatement
tests/scene_segments_ref.py.

Every comparison is bit for bit: the definition ("Pooling scores over segments") fixes every operation and
its order, so no tolerance is used in this file.  Where the defined result is a NaN (+inf and -inf in one column) the NaN
positions are compared and everything else bit for bit: the payload of a NaN differs between numpy and the device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_sets_ref  # noqa: E402
import scene_segments_ref as R  # noqa: E402

from r3dfsseg_amd import scene, scene_segments as SS  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
TOP = 2 ** 31 - 2  # the largest legal id
# members of the crafted segments: the tile edges, and one segment of eleven tiles
EDGE = [(0, 1), (255, 2), (256, 255), (65535, 256), (65536, 257), (2 ** 24, 512), (TOP, 513), (1000, 2600)]
FLOAT_FIELDS = ("scores", "segment_scores", "margin", "segment_margin")
INT_FIELDS = ("labels", "pooled", "segment_index", "segment_ids", "segment_points", "segment_members", "segment_labels",
              "set_labels", "set_of", "segment_set_labels", "segment_set_of")
COUNTS = ("n_segments", "n_pooled", "n_filled", "n_unlabelled")
_cache = {}


def _main_case(cols, top=TOP, negatives=True, seed=0):
    """(scores (M, cols), votes, labels, segments int64) of the main case, M about 6000, in a random scan order.  top: ids
    above it are replaced by small unused ones, so that the largest id -- and with it the number of radix passes -- varies."""
    key = ("main", cols, top, negatives, seed)
    if key in _cache:
        return _cache[key]
    rs = np.random.RandomState(seed)
    seg, votes, col0, ids = [], [], [], {}
    for n, (g0, members) in enumerate(EDGE):
        g = g0 if g0 <= top else 10 + n
        if g0 == 1000 and top not in [e[0] for e in EDGE]:
            g = top  # the largest id is `top` itself
        ids[g0] = g
        extra = (0, 3, 0, 5, 2, 0, 7, 40)[n]  # points of the segment without a vote: they receive, they do not contribute
        v = rs.randint(1, 6, members)
        pattern = np.full(members, np.nan, f32)
        if members == 257:  # the cancelling rows of the host test, in scan order, one vote each so that the row is the score
            v[:] = 1
            pattern = R.cancelling_rows(257)[:, 0]
        seg += [g] * (members + extra)
        votes += list(v) + [0] * extra
        col0 += list(pattern) + [np.nan] * extra
    seg += [7] * 5          # a segment whose points have no vote: no member
    votes += [0] * 5
    col0 += [np.nan] * 5
    n_neg = 900 if negatives else 0
    seg += list(-rs.randint(1, 5, n_neg))
    votes += list(rs.randint(0, 6, n_neg))
    col0 += [np.nan] * n_neg
    seg, votes, col0 = np.array(seg, np.int64), np.array(votes, np.int32), np.array(col0, f32)
    M = len(seg)
    # a random scan order that keeps the order inside a segment (the cancelling rows depend on it): every point draws a
    # position, and the points of a segment take the positions they drew in ascending order
    slots, dest = rs.permutation(M), np.empty(M, np.int64)
    for g in np.unique(seg):
        idx = np.flatnonzero(seg == g)
        dest[idx] = np.sort(slots[idx])
    perm = np.empty(M, np.int64)
    perm[dest] = np.arange(M)
    seg, votes, col0 = seg[perm], votes[perm], col0[perm]
    scores = (rs.randn(M, cols) * 3).astype(f32) * np.maximum(votes, 1)[:, None].astype(f32)
    scores[rs.rand(M, cols) < 0.02] = f32(-0.0)
    use = ~np.isnan(col0)
    scores[use, 0] = col0[use]
    big = np.flatnonzero((seg == ids[2 ** 24]) & (votes > 0))
    scores[big[3], cols - 1], scores[big[300], cols - 1] = f32(np.inf), f32(-np.inf)  # their sum is a NaN
    one = np.flatnonzero((seg == ids[256]) & (votes > 0))
    scores[one[100], cols - 1] = f32(np.inf)                                          # an infinite mean
    labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)
    _cache[key] = (scores, votes, labels, seg)
    return _cache[key]


def _want(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _same_float(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == f32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)), what


def _same(seg, want, sets=False):
    """Every field of a SegmentResult against the restatement's dict."""
    for name in FLOAT_FIELDS + INT_FIELDS:
        if name not in want:
            assert not sets and getattr(seg, name) is None, name
            continue
        got = getattr(seg, name).cpu().numpy()
        if name in FLOAT_FIELDS:
            _same_float(got, want[name], name)
        else:
            assert got.dtype == want[name].dtype and np.array_equal(got, want[name]), name
    assert {k: getattr(seg, k) for k in COUNTS} == {k: want[k] for k in COUNTS}


def _scene_result(scores, votes, labels):
    return scene.SceneResult(torch.from_numpy(labels).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(votes).cuda(),
                             1, 1, int((labels == -1).sum()), 0)


# ---- 1. the kernels against the restatement ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("cols", [2, 3, 12, 64])
def test_main_case_equals_the_restatement(cols, dtype):
    scores, votes, labels, seg = _main_case(cols)
    assert 5000 <= len(seg) <= 7000 and (seg < 0).sum() == 900 and seg.max() == TOP
    res = _scene_result(scores, votes, labels)
    segments = torch.from_numpy(seg).to(dtype)
    for mm in (1, 3):
        want = _want(("main-ref", cols, mm), lambda: R.pool(scores, votes, labels, seg, min_members=mm))
        got = SS.pool_segments(res, segments if mm == 1 else segments.cuda(), min_members=mm)  # host and device ids
        _same(got, want)
        assert got.votes is res.votes and got.source is None
    # what the case is there for
    members = dict(zip(want["segment_ids"].tolist(), want["segment_members"].tolist()))
    assert [members[g] for g, _ in EDGE] == [n for _, n in EDGE] and members[7] == 0
    row = want["segment_ids"].tolist().index
    assert want["segment_labels"][row(7)] == -1 and not want["segment_scores"][row(7)].any()
    assert want["segment_scores"][row(65536), 0] == f32(1) / f32(257)                  # the cancelling rows: 1, not 255
    assert np.isnan(want["segment_scores"][row(2 ** 24), cols - 1]) and np.isinf(want["segment_scores"][row(256), cols - 1])
    assert want["segment_labels"][row(256)] == cols - 1
    small = want["segment_index"] == row(255)                                          # 2 members < min_members = 3
    assert small.sum() == 5 and not want["pooled"][small].any() and _cache[("main-ref", cols, 1)]["pooled"][small].all()
    assert np.array_equal(want["scores"][small].view(np.uint32), scores[small].view(np.uint32))
    assert (np.signbit(scores) & (scores == 0)).any() and want["n_filled"] > 0


@pytest.mark.parametrize("top,negatives", [(255, False), (255, True), (256, True), (65535, False), (65535, True), (65536, True),
                                           (2 ** 24 - 1, False), (2 ** 24, True)])
def test_every_number_of_radix_passes(top, negatives):
    """The largest key decides the passes: 255 without a negative id is one pass, with one (their key is 256) two; 65535 two
    or three; 2^24 - 1 three, 2^24 four."""
    scores, votes, labels, seg = _main_case(3, top, negatives, seed=1)
    assert seg.max() == top and ((seg < 0).any() == negatives)
    want = R.pool(scores, votes, labels, seg)
    got = SS.pool_segments(_scene_result(scores, votes, labels), torch.from_numpy(seg))
    _same(got, want)
    assert got.n_segments == len(EDGE) + 1


@pytest.mark.parametrize("cols,dtype", [(3, torch.int32), (12, torch.int64)])
def test_many_sort_tiles(cols, dtype):
    """70 001 points, about 300 ids: the sort and the scans cross their 2048-element tiles."""
    rs = np.random.RandomState(cols)
    M = 70001
    ids = rs.choice(100000, 300, replace=False)
    seg = ids[(rs.rand(M) ** 2 * 300).astype(np.int64)].astype(np.int64)  # sizes from about 100 to about 4000
    seg[rs.rand(M) < 0.1] = -1
    votes = rs.randint(0, 6, M).astype(np.int32)
    scores = (rs.randn(M, cols).astype(f32) * np.maximum(votes, 1)[:, None].astype(f32))
    labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)
    want = R.pool(scores, votes, labels, seg, min_members=2)
    got = SS.pool_segments(_scene_result(scores, votes, labels), torch.from_numpy(seg).to(dtype).cuda(), min_members=2)
    _same(got, want)
    assert got.n_segments == 300 and want["segment_members"].max() > 256 > want["segment_members"].min()


def test_no_segment_at_all():
    scores, votes, labels, _ = _main_case(3)
    res = _scene_result(scores, votes, labels)
    seg = np.full(len(votes), -3, np.int64)
    got = SS.pool_segments(res, torch.from_numpy(seg))
    _same(got, R.pool(scores, votes, labels, seg))
    assert got.n_segments == 0 and got.n_pooled == 0 and torch.equal(got.scores, res.scores) and got.segment_scores.shape == (0, 3)


# ---- 2. ids that are refused ---------------------------------------------------------------------------------------------------
def test_ids_of_2_to_the_31_minus_1_and_more_are_refused():
    scores, votes, labels, seg = _main_case(3)
    res = _scene_result(scores, votes, labels)
    before = [t.clone() for t in (res.scores, res.votes, res.labels)]
    bad = torch.from_numpy(seg).to(torch.int32)
    bad[17] = 2 ** 31 - 1
    with pytest.raises(ValueError, match=r"1 segment ids are 2\^31 - 1 or more \(the largest: 2147483647\)"):
        SS.pool_segments(res, bad)
    bad = torch.from_numpy(seg).clone()
    bad[5], bad[4000], bad[4001] = 2 ** 40, 2 ** 31 - 1, 2 ** 33
    with pytest.raises(ValueError, match=r"3 segment ids are 2\^31 - 1 or more \(the largest: %d\)" % 2 ** 40):
        SS.pool_segments(res, bad.cuda())
    assert all(torch.equal(a, b) for a, b in zip(before, (res.scores, res.votes, res.labels)))
    _same(SS.pool_segments(res, torch.from_numpy(seg)), _want(("main-ref", 3, 1), lambda: R.pool(scores, votes, labels, seg)))


# ---- 3. a sets result ----------------------------------------------------------------------------------------------------------
def test_sets_result():
    from r3dfsseg_amd import ops
    K, C, classes, background = 3, 3, [[5, 6], [6, 7], [8, 9]], 0
    flat, votes, _, seg = _main_case(K * C, seed=2)
    M = len(votes)
    scores = flat.reshape(M, K, C)
    table = torch.tensor(classes, dtype=torch.int32).cuda()
    d_scores, d_votes = torch.from_numpy(scores).cuda(), torch.from_numpy(votes).cuda()
    set_labels, labels, set_of, margin = ops.scene_merge_sets(d_scores, d_votes, None, table, background)
    res = scene.SceneSetsResult(d_scores, set_labels, d_votes, labels, set_of, margin, 1, 1, int((votes == 0).sum()), 0)
    clones = [t.clone() for t in (res.scores, res.set_labels, res.votes, res.labels, res.set_of, res.margin)]
    for mm in (1, 3):
        got = SS.pool_segments(res, torch.from_numpy(seg), min_members=mm, classes=classes, background=background)
        want = R.pool(scores, votes, labels.cpu().numpy(), seg, min_members=mm, classes=np.array(classes, np.int32),
                      background=background, sets=(set_labels.cpu().numpy(), set_of.cpu().numpy(), margin.cpu().numpy()))
        _same(got, want, sets=True)
        assert got.scores.shape == (M, K, C) and got.segment_scores.shape == (got.n_segments, K, C)
        # the segment-level merge is scene_sets_ref's on the restated table
        sl, lab, so, mg = scene_sets_ref.merge(want["segment_scores"], want["segment_members"], None, np.array(classes), background)
        assert np.array_equal(got.segment_set_labels.cpu().numpy(), sl) and np.array_equal(got.segment_labels.cpu().numpy(), lab)
        assert np.array_equal(got.segment_set_of.cpu().numpy(), so)
        _same_float(got.segment_margin.cpu().numpy(), mg, "segment_margin")
        assert -1 in lab and set(np.unique(lab)) & {5, 6, 7, 8, 9}
        # the per-point fields are what the merge kernel gives on the per-point output
        has = (got.pooled | (res.votes > 0)).to(torch.int32)
        p_sl, p_lab, p_so, p_mg = ops.scene_merge_sets(got.scores, has, None, table, background)
        assert torch.equal(p_sl, got.set_labels) and torch.equal(p_lab, got.labels) and torch.equal(p_so, got.set_of)
        _same_float(p_mg.cpu().numpy(), got.margin.cpu().numpy(), "margin")
    assert all(torch.equal(a, b) for a, b in zip(clones, (res.scores, res.set_labels, res.votes, res.labels, res.set_of, res.margin)))
    with pytest.raises(ValueError, match="classes"):
        SS.pool_segments(res, torch.from_numpy(seg), classes=[[5, 6]])


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def _voxels(scan, size=0.25):
    xyz = scan[:, :3].cpu().numpy()
    c = np.floor((xyz - xyz.min(0)) / np.float32(size)).astype(np.int64)
    return (c[:, 2] * 64 + c[:, 1]) * 64 + c[:, 0]


def _tensors(res, sets):
    names = ("scores", "votes", "labels", "source", "neighbours", "weights") + (("set_labels", "set_of", "margin") if sets else ())
    return [(n, getattr(res, n)) for n in names if getattr(res, n) is not None]


def _pool_and_compare(learner, res, seg, sets=False, **kw):
    before = [(n, t, t.clone()) for n, t in _tensors(res, sets)]
    got = learner.pool_segments(res, torch.from_numpy(seg), **kw)
    ref_sets = (res.set_labels.cpu().numpy(), res.set_of.cpu().numpy(), res.margin.cpu().numpy()) if sets else None
    want = R.pool(res.scores.cpu().numpy(), res.votes.cpu().numpy(), res.labels.cpu().numpy(), seg, sets=ref_sets,
                  min_members=kw.get("min_members", 1),
                  classes=np.array(kw["classes"], np.int32) if kw.get("classes") is not None else None,
                  background=kw.get("background", -1))
    _same(got, want, sets=sets)
    for n, t, clone in before:                       # res is as it was
        assert torch.equal(t, clone) or (n in ("scores", "margin", "weights") and torch.equal(torch.isnan(t), torch.isnan(clone))), n
    keep = ~got.pooled                               # every point that is not pooled has the bits of res
    for n in ("scores", "labels") + (("set_labels", "set_of", "margin") if sets else ()):
        assert torch.equal(getattr(got, n)[keep].view(torch.uint8), getattr(res, n)[keep].view(torch.uint8)), n
    assert got.votes is res.votes and got.source is res.source and got.neighbours is res.neighbours and got.weights is res.weights
    return got


@pytest.mark.parametrize("cap,transfer", [(None, None), (1, None), (1, "nearest")])
def test_end_to_end_proto(cap, transfer):
    from test_gpu_scene import _learner, _room
    learner, cfg = _learner("proto")
    scan = _room(cfg)
    seg = _voxels(scan)
    assert 20 <= len(np.unique(seg)) <= 400
    res = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, max_chunks_per_block=cap, transfer=transfer)
    got = _pool_and_compare(learner, res, seg)
    assert got.n_pooled > 0 and got.n_segments == len(np.unique(seg))
    if cap == 1 and transfer is None:
        assert got.n_filled > 0 and got.n_unlabelled < res.n_unlabelled  # points of an object that had no vote get its label
    _pool_and_compare(learner, res, seg, min_members=4)


def test_end_to_end_sets():
    from test_gpu_scene import _room
    from test_gpu_scene_sets import SCENE, _learner
    learner, cfg, fits = _learner("proto")
    scan = _room(cfg)
    classes = [[5, 6], [6, 7], [8, 9]]
    res = learner.predict_scene_sets(scan, fits, classes=classes, background=0, **SCENE)
    got = _pool_and_compare(learner, res, _voxels(scan), sets=True, classes=classes, background=0)
    assert got.n_pooled > 0 and got.segment_set_labels.shape == (got.n_segments, 3)


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------
def test_two_calls_and_both_id_types_give_the_same_bits():
    scores, votes, labels, seg = _main_case(12)
    res = _scene_result(scores, votes, labels)
    a = SS.pool_segments(res, torch.from_numpy(seg))
    b = SS.pool_segments(res, torch.from_numpy(seg))
    c = SS.pool_segments(res, torch.from_numpy(seg).to(torch.int32).cuda())
    for other in (b, c):
        for name in ("scores", "labels", "pooled", "segment_index", "segment_ids", "segment_points", "segment_members",
                     "segment_scores", "segment_labels"):
            x, y = getattr(a, name), getattr(other, name)
            assert x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), name
        assert [getattr(a, k) for k in COUNTS] == [getattr(other, k) for k in COUNTS]
