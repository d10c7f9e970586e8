"""grow_segments (build_segments with normal_tol) on the device (r3dfsseg_amd/scene_grow.py, csrc/scene_grow.hip) against the numpy restatement
tests/scene_grow_normals_ref.py (which tests/test_scene_grow_normals_host.py checks against float64 eigenvectors and a
breadth-first search).

Every comparison is on integers or bit for bit on floats (torch.equal; a row of NaNs is compared by position, its payload is
not promised): the definition ("Building segments", G3c, G3n, G4) fixes every operation and its order, so no
tolerance is used in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_grow_cases as C  # noqa: E402
import scene_grow_normals_cases as NC  # noqa: E402
import scene_grow_normals_ref as N  # noqa: E402

from r3dfsseg_amd import fitted, ops, scene_grow as G  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
INT_FIELDS = ("segments", "segment_points", "voxel_index")
COUNTS = ("n_segments", "n_voxels", "n_components", "n_dropped_points", "n_invalid")
TABLES = ("voxel_means", "voxel_centroids", "voxel_normals")
_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _want(name, scan, voxel, colour_tol, connectivity, min_points, normal_tol):
    """The restatement of a named case, computed once."""
    return _cached(("ref", name, voxel, colour_tol, connectivity, min_points, normal_tol),
                   lambda: N.grow(scan, voxel, colour_tol, connectivity, min_points, normal_tol=normal_tol))


def _same_floats(got, want, name):
    """got: a device tensor, want: a numpy array; NaNs by position, everything else by torch.equal."""
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, name
    assert torch.equal(torch.isnan(got), torch.isnan(want)), name
    zero = torch.zeros((), dtype=torch.float32)
    assert torch.equal(torch.where(torch.isnan(got), zero, got), torch.where(torch.isnan(want), zero, want)), name


def _same(got, want):
    """Every field of a GrownSegments against the restatement's dict."""
    for name in INT_FIELDS:
        assert torch.equal(getattr(got, name).cpu(), torch.from_numpy(want[name])) and want[name].dtype == np.int32, name
    assert {k: getattr(got, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert got.grid == want["grid"]
    for name in TABLES:
        if want.get(name) is None:
            assert getattr(got, name) is None, name
        else:
            _same_floats(getattr(got, name), want[name], name)
    if want["voxel_support"] is None:
        assert got.voxel_support is None
    else:
        assert got.voxel_support.dtype == torch.int32 and torch.equal(got.voxel_support.cpu(), torch.from_numpy(want["voxel_support"]))


def _check(name, scan, voxel, colour_tol, connectivity, min_points=1, normal_tol=10.0):
    want = _want(name, scan, voxel, colour_tol, connectivity, min_points, normal_tol)
    got = G.grow_segments(scan, voxel=voxel, colour_tol=colour_tol, connectivity=connectivity, min_points=min_points,
                           normal_tol=normal_tol)
    _same(got, want)
    return got, want


# ---- 1. two planes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("colour_tol", [None, 0.125])
def test_two_perpendicular_planes_are_two_segments(colour_tol, connectivity):
    """A floor and a wall of 30 x 30 voxels that share an edge: one component by adjacency, two (and the voxels of the edge)
    with normals, with and without the colour test (the planes differ in colour by 0.5, so colour_tol 0.125 parts them
    too; it changes nothing here and must change nothing)."""
    scan, coords = _cached("planes", NC.two_planes_case)
    got, want = _check("planes", scan, 0.05, colour_tol, connectivity)
    assert got.grid == (30, 30, 30) and got.n_voxels == 900 + 870
    seg = got.segments.cpu().numpy()
    floor, wall = (coords[:, 2] == 0) & (coords[:, 0] >= 2), (coords[:, 0] == 0) & (coords[:, 2] >= 2)
    assert len(set(seg[floor])) == 1 and len(set(seg[wall])) == 1 and seg[floor][0] != seg[wall][0] and seg[floor][0] >= 0
    n = got.voxel_normals[got.voxel_index.long()].cpu().numpy()
    assert (n[floor] == [0, 0, 1]).all() and (n[wall] == [1, 0, 0]).all()
    if colour_tol is None:
        assert G.build_segments(scan, connectivity=connectivity).n_components == 1


# ---- 2. small neighbourhoods, the borders of the grid ------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_voxels_with_few_neighbours(connectivity):
    """A lone voxel and a line of three have no normal (support 1 and 2, 3, 2) and stay alone; a flat patch of exactly four
    has one, (0, 0, 1), and is one component."""
    scan, coords = _cached("small", NC.small_case)
    got, want = _check("small", scan, C.VOX, None, connectivity)
    row = lambda v: int(got.voxel_index[np.flatnonzero((coords == v).all(1))[0]])
    sup, nrm, comp = got.voxel_support.cpu().numpy(), got.voxel_normals.cpu().numpy(), want["voxel_component"]
    assert sup[row(NC.SMALL_LONE[0])] == 1 and [sup[row(v)] for v in NC.SMALL_LINE] == [2, 3, 2]
    for v in NC.SMALL_LONE + NC.SMALL_LINE:
        assert np.isnan(nrm[row(v)]).all() and (comp == comp[row(v)]).sum() == 1
    assert all(sup[row(v)] == 4 and nrm[row(v)].tolist() == [0, 0, 1] for v in NC.SMALL_PATCH)
    seg = got.segments.cpu().numpy()
    assert len({seg[np.flatnonzero((coords == v).all(1))[0]] for v in NC.SMALL_PATCH}) == 1


@pytest.mark.parametrize("connectivity", [6, 26])
def test_consecutive_keys_across_a_row_or_a_slab_are_no_neighbours(connectivity):
    """The sparse 5 x 4 x 3 case of the adjacency tests: the last voxel of a row and the first of the next have consecutive
    keys and are no neighbours, so every support is at most 2 and no voxel has a normal."""
    scan, coords = _cached("wrap", C.wrap_case)
    got, want = _check("wrap", scan, C.VOX, None, connectivity)
    assert got.grid == C.WRAP_GRID and got.n_voxels == got.n_components == 7
    assert sorted(got.voxel_support.tolist()) == [1, 1, 1, 1, 1, 2, 2] and torch.isnan(got.voxel_normals).all()


@pytest.mark.parametrize("share", [0.1, 0.5, 1.0])
def test_centroids_normals_and_support_on_random_occupancy(share):
    """12 x 11 x 10 voxels, 10 %, 50 % and all of them occupied (all: every face, edge and corner of the grid, and every
    row's last voxel followed in the table by the next row's first): the two new launches alone, through the ops wrappers."""
    scan, _ = _cached(("occupancy", share), lambda: NC.occupancy_case(share))
    want = _want(("occupancy", share), scan, C.VOX, None, 26, 1, 10.0)
    assert want["grid"] == (12, 11, 10) and abs(want["n_voxels"] / 1320 - share) < 0.05
    if share == 1.0:
        assert np.bincount(want["voxel_support"], minlength=28)[[8, 12, 18, 27]].tolist() == [8, 4 * (10 + 9 + 8), 2 * (90 + 80 + 72), 720]
    dev = torch.from_numpy(scan).cuda()
    ws, lo, grid, V, voxel_index, _ = _tables(dev, C.VOX, False)
    centroids = ops.scene_grow_centroids(dev, lo, f32(C.VOX), grid, V, ws)
    normals, support = ops.scene_grow_normals(len(scan), grid, V, f32(C.VOX), centroids, ws)
    assert V == want["n_voxels"] and torch.equal(voxel_index.cpu(), torch.from_numpy(want["voxel_index"]))
    _same_floats(centroids, want["voxel_centroids"], "centroids")
    _same_floats(normals, want["voxel_normals"], "normals")
    assert torch.equal(support.cpu(), torch.from_numpy(want["voxel_support"]))
    assert -1e-5 <= float(centroids.min()) and float(centroids.max()) <= C.VOX + 1e-5  # inside the voxel, up to rounding
    _check(("occupancy", share), scan, C.VOX, None, 26)


# ---- 3. the summation order, a long axis ---------------------------------------------------------------------------------------
def test_the_centroids_of_voxels_of_257_and_2600_points():
    """(tests/test_scene_grow_normals_host.py shows that the reverse order, one running sum and the exact sum give other
    centroids for these two voxels.)"""
    scan, coords = _cached("big", NC.big_voxel_case)
    got, want = _check("big", scan, 0.05, None, 6)
    assert sorted(want["voxel_points"].tolist())[-2:] == [257, 2600] and got.n_voxels == 15


@pytest.mark.parametrize("axis", [0, 2])
def test_an_axis_of_1024_voxels(axis):
    scan, _ = _cached(("strip", axis), lambda: NC.strip_case(axis))
    got, want = _check(("strip", axis), scan, 0.05, None, 6)
    assert got.grid == ((1024, 2, 1) if axis == 0 else (1, 2, 1024)) and got.n_voxels == 2048
    assert got.n_components == 1 and got.voxel_support.min() == 4 and got.voxel_support.max() == 6
    assert not torch.isnan(got.voxel_normals).any()


# ---- 4. tolerances, colour, min_points, invalid points ---------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("normal_tol", [0, 10, 90])
def test_tolerances(normal_tol, connectivity):
    scan, _ = _cached(("random", 0), lambda: C.random_case(0))
    got, want = _check(("random", 0), scan, 0.05, None, connectivity, normal_tol=normal_tol)
    plain = _cached(("plain", connectivity), lambda: G.build_segments(scan, connectivity=connectivity).n_components)
    assert got.n_components > plain  # also at 90 degrees: a voxel without a normal joins nothing
    assert torch.isnan(got.voxel_normals[:, 0]).sum() > 0
    if normal_tol == 90:
        assert got.n_components < _want(("random", 0), scan, 0.05, None, connectivity, 1, 10)["n_components"]


@pytest.mark.parametrize("colour_tol,connectivity", [(0.5, 6), (0.25, 26)])
def test_with_colour_tol_both_tests_must_hold(colour_tol, connectivity):
    scan, _ = _cached(("random", 1), lambda: C.random_case(1))
    got, want = _check(("random", 1), scan, 0.05, colour_tol, connectivity, normal_tol=30.0)
    only_normals = _want(("random", 1), scan, 0.05, None, connectivity, 1, 30.0)["n_components"]
    only_colour = G.build_segments(scan, colour_tol=colour_tol, connectivity=connectivity).n_components
    assert got.n_components > max(only_normals, only_colour) and got.voxel_means is not None


@pytest.mark.parametrize("connectivity", [6, 26])
def test_invalid_points_and_min_points(connectivity):
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    bad = ~np.isfinite(scan[:, :3]).all(1)
    got, want = _check("invalid", scan, 0.05, None, connectivity, normal_tol=30.0)
    assert got.n_invalid == bad.sum() > 100 and (got.segments.cpu().numpy()[bad] == -1).all() and got.n_dropped_points == 0
    sizes = np.sort(want["segment_points"])
    size = int(sizes[-3])
    assert sizes[0] < size - 1 and size + 1 <= sizes[-1]
    for mp in (size - 1, size, size + 1):  # below, at and above the size of a component
        g, _ = _check("invalid", scan, 0.05, None, connectivity, min_points=mp, normal_tol=30.0)
        assert g.n_segments == int((sizes >= mp).sum()) and g.n_components == got.n_components
        assert g.n_dropped_points == int(sizes[sizes < mp].sum()) > 0
    g, _ = _check("invalid", scan, 0.05, None, connectivity, min_points=int(sizes[-1]) + 1, normal_tol=30.0)
    assert g.n_segments == 0 and (g.segments == -1).all() and g.voxel_normals.shape == (g.n_voxels, 3)


def test_only_invalid_points_and_a_single_point():
    scan = np.full((300, 3), np.nan, f32)
    got, _ = _check("all-invalid", scan, 0.05, None, 6)
    assert got.n_invalid == 300 and got.n_voxels == 0
    assert got.voxel_normals.shape == got.voxel_centroids.shape == (0, 3) and got.voxel_support.shape == (0,)
    one = np.array([[3.0, -1.0, 2.0]], f32)
    got, _ = _check("one", one, 0.05, None, 26)
    assert got.segments.tolist() == [0] and got.voxel_support.tolist() == [1] and got.voxel_centroids.tolist() == [[0.0, 0.0, 0.0]]
    assert torch.isnan(got.voxel_normals).all()


# ---- 5. promises -----------------------------------------------------------------------------------------------------------
def _fields(got):
    out = [getattr(got, k).cpu().numpy() for k in INT_FIELDS + ("voxel_support",)] + [[getattr(got, k) for k in COUNTS]]
    return out + [getattr(got, k).cpu().numpy().view(np.uint32) for k in TABLES if getattr(got, k) is not None]


@pytest.mark.parametrize("colour_tol,connectivity", [(None, 6), (0.5, 26)])
def test_two_calls_give_the_same_bits(colour_tol, connectivity):
    """NaN payloads included: the two calls run the same code."""
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    dev = torch.from_numpy(scan).cuda()
    a = G.grow_segments(dev, colour_tol=colour_tol, connectivity=connectivity, min_points=5, normal_tol=20.0)
    b = G.grow_segments(dev, colour_tol=colour_tol, connectivity=connectivity, min_points=5, normal_tol=20.0)
    c = G.grow_segments(scan, colour_tol=colour_tol, connectivity=connectivity, min_points=5, normal_tol=20.0)  # from the host
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(other)))


def test_a_host_scan_of_three_columns_equals_a_device_scan_of_six():
    scan = _cached(("random", 1), lambda: C.random_case(1))[0]
    a = G.grow_segments(np.ascontiguousarray(scan[:, :3]), connectivity=26, normal_tol=10.0)
    b = G.grow_segments(torch.from_numpy(scan).cuda(), connectivity=26, normal_tol=10.0)
    learner = fitted.FittedLearner.__new__(fitted.FittedLearner)  # the forwards need no model
    c = learner.grow_segments(scan, connectivity=26, normal_tol=10.0)
    assert a.voxel_means is None and a.n_components > 10
    for other in (b, c):
        assert all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(other)))
    _same(a, _want(("random", 1), scan, 0.05, None, 26, 1, 10.0))


def test_without_normal_tol_nothing_new_is_launched(monkeypatch):
    scan, _ = _cached(("random", 0), lambda: C.random_case(0))
    before = G.build_segments(scan, colour_tol=0.5, connectivity=26)

    def never(*a, **k):
        raise AssertionError("a normal_tol entry point was called without normal_tol")
    for name in ("scene_grow_centroids", "scene_grow_normals", "scene_grow_union_normals"):
        monkeypatch.setattr(ops, name, never)
    got = G.grow_segments(scan, colour_tol=0.5, connectivity=26, normal_tol=None)
    assert got.voxel_centroids is None and got.voxel_normals is None and got.voxel_support is None
    _same(got, N.grow(scan, 0.05, 0.5, 26))
    assert torch.equal(got.segments, before.segments)
    with pytest.raises(AssertionError, match="normal_tol entry point"):
        G.grow_segments(scan, normal_tol=10.0)


# ---- 6. the union entry point on hand-made normal tables ---------------------------------------------------------------------
def _tables(dev_scan, voxel, colour):
    """The steps of build_segments in front of the union, through the ops wrappers -> (ws, lo, grid, V, voxel_index, means)."""
    M = dev_scan.shape[0]
    ws = ops.scene_grow_workspace(M, dev_scan.device)
    ops.scene_grow_bounds(dev_scan, ws)
    rec = G.read_record(ws)
    ext = np.array(rec[ops.GROW_R_MIN:ops.GROW_R_MIN + 6], np.int32).view(f32)
    lo, hi = ext[:3], ext[3:]
    grid = G.grid_of(lo, hi, f32(voxel))
    ops.scene_grow_sort(dev_scan, lo, f32(voxel), grid, ws)
    V = G.read_record(ws)[ops.GROW_R_V]
    voxel_index, means = ops.scene_grow_voxels(dev_scan, grid, rec[ops.GROW_R_NVALID], V, colour, ws)
    return ws, lo, grid, V, voxel_index, means


def _union_with(scan, voxel, table, cos2, connectivity, colour_tol=None):
    """The components of a scan whose normal table is `table` (V, 3), not its own -> (segments, segment_points, record)."""
    dev = torch.from_numpy(scan).cuda()
    ws, lo, grid, V, voxel_index, means = _tables(dev, voxel, colour_tol is not None)
    assert V == len(table)
    ops.scene_grow_union_normals(len(scan), grid, V, connectivity, means, colour_tol, torch.from_numpy(table).cuda(), cos2, ws)
    ops.scene_grow_components(len(scan), V, 1, ws)
    rec = G.read_record(ws)
    segments, points = ops.scene_grow_ids(voxel_index, V, rec[ops.GROW_R_S], ws)
    return segments, points, G.read_record(ws)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_union_decides_at_the_threshold(connectivity):
    """Pairs of voxels with hand-made rows (tests/scene_grow_normals_cases.py, PAIRS) at cos2 = 0.5: dot^2 exactly equal to
    (cos2 la) lb joins, one ulp below does not; signs and lengths do not matter; a NaN joins nothing; an infinite row and a row
    of zeros go by the comparison alone (inf >= inf and 0 >= 0 are true: they join; inf * 0 is a NaN: no join)."""
    scan, coords, table, joined = _cached("pairs", NC.pairs_case)
    want = _cached(("pairs-ref", connectivity), lambda: N.grow(scan, C.VOX, None, connectivity, 1, normals=table, cos2=NC.COS2))
    segments, points, rec = _union_with(scan, C.VOX, table, NC.COS2, connectivity)
    assert rec[ops.GROW_R_ERROR] == 0 and rec[ops.GROW_R_NCOMP] == want["n_components"] == 2 * len(joined) - sum(joined)
    assert torch.equal(segments.cpu(), torch.from_numpy(want["segments"])) and torch.equal(points.cpu(), torch.from_numpy(want["segment_points"]))
    seg = segments.cpu().numpy()
    of = lambda x: seg[np.flatnonzero(coords[:, 0] == x)[0]]
    assert [bool(of(3 * p) == of(3 * p + 1)) for p in range(len(joined))] == joined


@pytest.mark.parametrize("connectivity", [6, 26])
def test_a_full_grid_of_equal_normals_is_one_component(connectivity):
    """65 536 voxels whose rows are one direction at lengths 2^-8 .. 2^8 and either sign: every thread of the union kernel
    hooks into the same tree, the error word stays 0; with cos2 = 1 the rows still join (the products are exact)."""
    scan, _ = _cached(("full", None), lambda: C.full_grid_case(None))
    rs = np.random.RandomState(41)
    table = (np.array([[0.25, -0.5, 1.0]], f32) * (np.exp2(rs.randint(-8, 9, 65536)) * rs.choice([-1.0, 1.0], 65536))[:, None]).astype(f32)
    segments, points, rec = _union_with(scan, C.VOX, table, f32(1.0), connectivity)
    assert rec[ops.GROW_R_ERROR] == 0 and rec[ops.GROW_R_NCOMP] == rec[ops.GROW_R_S] == 1
    assert points.tolist() == [65536] and not segments.any()
    table[40000] = np.nan  # one voxel without a normal: a component of its own
    segments, points, rec = _union_with(scan, C.VOX, table, f32(1.0), connectivity)
    assert rec[ops.GROW_R_ERROR] == 0 and rec[ops.GROW_R_NCOMP] == 2 and sorted(points.tolist()) == [1, 65535]


def test_the_union_with_hand_made_normals_and_colour():
    scan, _ = _cached(("random", 0), lambda: C.random_case(0))
    own = _want(("random", 0), scan, 0.05, None, 26, 1, 10)
    rs = np.random.RandomState(42)
    table = rs.randn(own["n_voxels"], 3).astype(f32)
    table[rs.rand(len(table)) < 0.05] = np.nan
    want = N.grow(scan, 0.05, 0.5, 26, 1, normals=table, cos2=f32(0.25))
    segments, points, rec = _union_with(scan, 0.05, table, f32(0.25), 26, colour_tol=0.5)
    assert rec[ops.GROW_R_ERROR] == 0 and rec[ops.GROW_R_NCOMP] == want["n_components"] > 100
    assert torch.equal(segments.cpu(), torch.from_numpy(want["segments"])) and torch.equal(points.cpu(), torch.from_numpy(want["segment_points"]))
