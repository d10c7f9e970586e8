"""build_segments on the device (r3dfsseg_amd/scene_grow.py, csrc/scene_grow.hip) against the numpy restatement
tests/scene_grow_ref.py (which tests/test_scene_grow_host.py checks against a breadth-first search).

Every comparison is on integers, and bit for bit on the voxels' mean colours (a NaN mean: the NaN positions): the definition
("Building segments") fixes every operation and its order, so no tolerance is used in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_grow_cases as C  # noqa: E402
import scene_grow_ref as R  # noqa: E402
import scene_segments_ref  # noqa: E402

from r3dfsseg_amd import fitted, scene, scene_grow as G, scene_segments as SS  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
INT_FIELDS = ("segments", "segment_points", "voxel_index")
COUNTS = ("n_segments", "n_voxels", "n_components", "n_dropped_points", "n_invalid")
_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _want(name, scan, voxel, colour_tol, connectivity, min_points=1):
    """The restatement of a named case, computed once."""
    return _cached(("ref", name, voxel, colour_tol, connectivity, min_points),
                   lambda: R.grow(scan, voxel, colour_tol, connectivity, min_points))


def _same(got, want):
    """Every field of a GrownSegments against the restatement's dict."""
    for name in INT_FIELDS:
        a = getattr(got, name).cpu().numpy()
        assert a.dtype == want[name].dtype == np.int32 and np.array_equal(a, want[name]), name
    assert {k: getattr(got, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert got.grid == want["grid"]
    if want.get("voxel_means") is None:
        assert got.voxel_means is None or got.n_voxels == 0
    else:
        a, b = got.voxel_means.cpu().numpy(), want["voxel_means"]
        assert a.shape == b.shape and a.dtype == b.dtype == f32
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _check(name, scan, voxel, colour_tol, connectivity, min_points=1):
    want = _want(name, scan, voxel, colour_tol, connectivity, min_points)
    got = G.build_segments(scan, voxel=voxel, colour_tol=colour_tol, connectivity=connectivity, min_points=min_points)
    _same(got, want)
    return got, want


# ---- 1. rows and slabs whose keys are consecutive ------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_consecutive_keys_across_a_row_or_a_slab_are_no_neighbours(connectivity):
    scan, coords = _cached("wrap", C.wrap_case)
    assert np.array_equal(scan[:, :3].max(0), scan[(coords == C.WRAP_CORNER).all(1)][0, :3])  # a point at the exact maximum
    got, want = _check("wrap", scan, C.VOX, None, connectivity)
    assert got.grid == C.WRAP_GRID and got.n_voxels == 7 and got.n_components == 6
    seg = got.segments.cpu().numpy()
    of = lambda v: seg[np.flatnonzero((coords == v).all(1))[0]]
    for a, b in C.WRAP_PAIRS:
        assert of(a) != of(b)
    assert of((4, 3, 1)) == of(C.WRAP_CORNER)


# ---- 2. long thin components -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_serpentines(connectivity):
    """Two one-voxel-wide paths of 272 and 273 voxels in a 33 x 33 x 1 grid that share a corner and no face, scan rows
    shuffled: two components by faces, one with corners.  (Two such paths cannot both be 500 voxels long in this grid: with
    a free line between their turns they hold about 580 voxels together.)"""
    scan, coords = _cached("serpentine", C.serpentine_case)
    got, want = _check("serpentine", scan, C.VOX, None, connectivity)
    assert got.grid == (33, 33, 1) and got.n_voxels == 545
    assert got.n_components == got.n_segments == (2 if connectivity == 6 else 1)
    if connectivity == 6:
        assert sorted(got.segment_points.tolist()) == [3 * 272, 3 * 273]


# ---- 3. contention ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("without_plane", [None, 8])
def test_a_full_grid_is_one_component(without_plane, connectivity):
    """65 536 voxels of one point each: every thread of the union kernel hooks into the same tree; 64 * 64 * 16 = 2^16 cells
    take three radix passes."""
    scan, coords = _cached(("full", without_plane), lambda: C.full_grid_case(without_plane))
    got, _ = _check(("full", without_plane), scan, C.VOX, None, connectivity)
    M = len(scan)
    assert M == 65536 - (0 if without_plane is None else 4096)
    assert got.grid == (64, 64, 16) and got.n_voxels == M and got.n_invalid == 0 and got.n_dropped_points == 0
    # and in closed form: the voxel table is the grid in key order, the components are the slabs
    keys = (coords[:, 2] * 64 + coords[:, 1]) * 64 + coords[:, 0]
    rows = np.searchsorted(np.sort(keys), keys)
    assert np.array_equal(got.voxel_index.cpu().numpy(), rows.astype(np.int32))
    seg = got.segments.cpu().numpy()
    if without_plane is None:
        assert got.n_components == got.n_segments == 1 and not seg.any() and got.segment_points.tolist() == [M]
    else:
        assert got.n_components == got.n_segments == 2 and np.array_equal(seg, (coords[:, 2] > 8).astype(np.int32))
        assert got.segment_points.tolist() == [8 * 4096, 7 * 4096]


# ---- 4. colour -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_colour_decides_at_the_tolerance_in_every_channel(connectivity):
    scan, coords = _cached("colour-line", C.colour_line_case)
    got, want = _check("colour-line", scan, C.VOX, C.COLOUR_TOL, connectivity)
    assert got.n_components == 3 * len(C.COLOUR_LINE_PARTS) and got.n_dropped_points == 0
    seg = got.segments.cpu().numpy()
    for c in range(3):
        line = [seg[np.flatnonzero((coords[:, 0] == x) & (coords[:, 1] == 2 * c))[0]] for x in range(8)]
        assert [sorted(x for x in range(8) if line[x] == s) for s in sorted(set(line))] == C.COLOUR_LINE_PARTS
        assert line[5] >= 0  # the voxel with a NaN colour joins nothing and keeps its point
    assert np.isnan(got.voxel_means.cpu().numpy()).sum() == 3
    _check("colour-line", scan, C.VOX, None, connectivity)
    _check("colour-line", scan[:, :3].copy(), C.VOX, None, connectivity)


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_the_summation_order_of_a_voxel_decides_the_join(channel):
    """Voxels of 257 and 2600 points with cancelling colours, each beside a voxel that holds the mean G3 defines; with
    colour_tol = 0 they join only when the device adds in G3's order (tests/test_scene_grow_host.py shows that a running sum,
    the reverse order and the exact sum all give another mean)."""
    scan, coords, means = _cached(("cancel", channel), lambda: C.cancelling_case(channel))
    got, want = _check(("cancel", channel), scan, C.VOX, 0.0, 6)
    assert got.n_voxels == 4 and got.n_components == 2 and want["voxel_component"].tolist() == [0, 0, 2, 2]
    m = got.voxel_means.cpu().numpy()[:, channel]
    assert m[0] == m[1] == means[0] == f32(1) / f32(257) and m[2] == m[3] == means[1] == f32(2344) / f32(2600)


# ---- 5. random -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour_tol,connectivity", [(None, 6), (0.5, 26)])
@pytest.mark.parametrize("seed", [0, 1])
def test_random_grids(seed, colour_tol, connectivity):
    scan, _ = _cached(("random", seed), lambda: C.random_case(seed))
    want = _want(("random", seed), scan, 0.05, colour_tol, connectivity)
    assert want["n_components"] >= 50 and np.bincount(want["voxel_component"]).max() >= 1000 and want["grid"] == (8, 24, 24)
    _check(("random", seed), scan, 0.05, colour_tol, connectivity)


# ---- 6. invalid points and small components -------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour_tol,connectivity", [(None, 6), (0.5, 26)])
def test_invalid_points_and_min_points(colour_tol, connectivity):
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    bad = ~np.isfinite(scan[:, :3]).all(1)
    assert 100 < bad.sum() and np.isnan(scan[:, :3]).any() and (scan[:, :3] == np.inf).any() and (scan[:, :3] == -np.inf).any()
    got, want = _check("invalid", scan, 0.05, colour_tol, connectivity)
    assert got.n_invalid == bad.sum() and (got.segments.cpu().numpy()[bad] == -1).all() and got.n_dropped_points == 0
    assert (got.voxel_index.cpu().numpy()[bad] == -1).all()
    sizes = np.sort(want["segment_points"])
    second, largest = int(sizes[-2]), int(sizes[-1])
    assert second < largest
    got2, want2 = _check("invalid", scan, 0.05, colour_tol, connectivity, min_points=second)
    assert got2.n_segments == int((sizes >= second).sum()) and got2.n_components == got.n_components
    assert got2.n_dropped_points == int(sizes[sizes < second].sum()) > 0
    got3, _ = _check("invalid", scan, 0.05, colour_tol, connectivity, min_points=largest + 1)
    assert got3.n_segments == 0 and got3.segment_points.numel() == 0 and (got3.segments == -1).all()
    assert got3.n_dropped_points == len(scan) - bad.sum()
    # pool_segments on a partition without a segment pools nothing
    rs = np.random.RandomState(3)
    M = len(scan)
    res = _scene_result(rs.randn(M, 3).astype(f32), rs.randint(0, 3, M).astype(np.int32))
    seg = SS.pool_segments(res, got3.segments)
    assert seg.n_segments == 0 and seg.n_pooled == 0 and not seg.pooled.any() and torch.equal(seg.scores, res.scores)


def test_only_invalid_points_and_a_single_point():
    scan = np.full((300, 6), np.nan, f32)
    scan[::3, 0], scan[1::3, 1] = np.inf, -np.inf
    scan[2::3, :3] = [[1.0, np.nan, 2.0]]
    for tol in (None, 0.1):
        got, _ = _check("all-invalid", scan, 0.05, tol, 6)
        assert got.n_invalid == 300 and got.n_segments == got.n_voxels == 0 and (got.segments == -1).all()
    one = np.array([[3.0, -1.0, 2.0, 0.5, 0.25, 1.0]], f32)
    got, _ = _check("one", one, 0.05, 0.1, 26)
    assert got.segments.tolist() == [0] and got.segment_points.tolist() == [1] and got.voxel_index.tolist() == [0]
    assert got.voxel_means.tolist() == [[0.5, 0.25, 1.0]] and got.grid == (1, 1, 1)
    got, _ = _check("one", one, 0.05, None, 6, min_points=2)
    assert got.segments.tolist() == [-1] and got.n_dropped_points == 1 and got.n_components == 1


# ---- 7. promises -----------------------------------------------------------------------------------------------------------
def _fields(got):
    out = [getattr(got, k).cpu().numpy() for k in INT_FIELDS] + [[getattr(got, k) for k in COUNTS]]
    return out + ([] if got.voxel_means is None else [got.voxel_means.cpu().numpy().view(np.uint32)])


@pytest.mark.parametrize("colour_tol,connectivity", [(None, 6), (0.5, 26)])
def test_two_calls_give_the_same_bits(colour_tol, connectivity):
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    dev = torch.from_numpy(scan).cuda()
    a = G.build_segments(dev, colour_tol=colour_tol, connectivity=connectivity, min_points=5)
    b = G.build_segments(dev, colour_tol=colour_tol, connectivity=connectivity, min_points=5)
    c = G.build_segments(scan, colour_tol=colour_tol, connectivity=connectivity, min_points=5)  # from the host
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(other)))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_a_permuted_scan_gives_the_permuted_segments(connectivity):
    """Without colour the partition does not depend on the order of the rows; the ids do not either: a component is numbered
    by its smallest voxel key."""
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    perm = np.random.RandomState(12).permutation(len(scan))
    a = G.build_segments(scan, connectivity=connectivity, min_points=3)
    b = G.build_segments(scan[perm], connectivity=connectivity, min_points=3)
    assert torch.equal(a.segments[torch.from_numpy(perm).cuda()], b.segments)
    assert torch.equal(a.voxel_index[torch.from_numpy(perm).cuda()], b.voxel_index)
    assert torch.equal(a.segment_points, b.segment_points)
    assert [getattr(a, k) for k in COUNTS] == [getattr(b, k) for k in COUNTS]


def test_a_host_scan_of_three_columns_equals_a_device_scan_of_six():
    scan = _cached(("random", 1), lambda: C.random_case(1))[0]
    a = G.build_segments(np.ascontiguousarray(scan[:, :3]), connectivity=26)
    b = G.build_segments(torch.from_numpy(scan).cuda(), connectivity=26)
    wide = np.concatenate([scan, np.ones((len(scan), 70), f32)], 1)  # more columns than a kernel row holds: six are read
    c = G.build_segments(wide, connectivity=26)
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(other)))
    assert a.voxel_means is None


# ---- 8. composition ----------------------------------------------------------------------------------------------------------
def _scene_result(scores, votes):
    labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)
    return scene.SceneResult(torch.from_numpy(labels).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(votes).cuda(),
                             1, 1, int((labels == -1).sum()), 0)


def test_pool_segments_takes_the_grown_segments_as_they_are():
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    want = _want("invalid", scan, 0.05, 0.5, 26, 4)
    M = len(scan)
    rs = np.random.RandomState(4)
    votes = rs.randint(0, 4, M).astype(np.int32)
    scores = (rs.randn(M, 5) * 3).astype(f32) * np.maximum(votes, 1)[:, None].astype(f32)
    res = _scene_result(scores, votes)
    learner = fitted.FittedLearner.__new__(fitted.FittedLearner)  # the forwards need no model
    sg = learner.build_segments(scan, colour_tol=0.5, connectivity=26, min_points=4)
    _same(sg, want)
    assert sg.n_segments > 10 and sg.n_dropped_points > 0
    a = learner.pool_segments(res, sg.segments)
    b = SS.pool_segments(res, torch.from_numpy(want["segments"]))
    assert a.n_segments == b.n_segments == sg.n_segments
    assert torch.equal(a.segment_points, sg.segment_points)
    for name in ("labels", "pooled", "segment_index", "segment_ids", "segment_points", "segment_members", "segment_labels"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("scores", "segment_scores"):
        assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), name
    assert (a.n_pooled, a.n_filled, a.n_unlabelled) == (b.n_pooled, b.n_filled, b.n_unlabelled)
    ref = scene_segments_ref.pool(scores, votes, res.labels.cpu().numpy(), want["segments"])
    assert np.array_equal(a.labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(a.segment_scores.cpu().numpy().view(np.uint32), ref["segment_scores"].view(np.uint32))
