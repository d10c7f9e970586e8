"""absorb_segments (grow_segments with absorb) on the device (r3dfsseg_amd/scene_grow.py, csrc/scene_grow.hip) against the numpy restatement
tests/scene_grow_absorb_ref.py (which tests/test_scene_grow_absorb_host.py checks against a breadth-first distance).

G6a ("Building segments") is integer work, so every comparison is exact: every field of the result, the
new ones included, equals the restatement's, for every case and ring count below."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_grow_absorb_cases as AC  # noqa: E402
import scene_grow_absorb_ref as A  # noqa: E402
import scene_grow_cases as C  # noqa: E402
import scene_grow_normals_cases as NC  # noqa: E402
import scene_grow_normals_ref as N  # noqa: E402

from r3dfsseg_amd import fitted, ops, scene, scene_grow as G, scene_segments as SS  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
INT_FIELDS = ("segments", "segment_points", "voxel_index")
COUNTS = ("n_segments", "n_voxels", "n_components", "n_dropped_points", "n_invalid", "n_absorbed_voxels", "n_absorbed_points")
TABLES = ("voxel_means", "voxel_centroids", "voxel_normals")
_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _base(name, scan, voxel, colour_tol, connectivity, min_points, normal_tol):
    """The restatement of a named case without absorb, computed once and left unchanged."""
    return _cached(("base", name, voxel, colour_tol, connectivity, min_points, normal_tol),
                   lambda: N.grow(scan, voxel, colour_tol, connectivity, min_points, normal_tol=normal_tol))


def _same_floats(got, want, name):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, name
    assert torch.equal(torch.isnan(got), torch.isnan(want)), name
    zero = torch.zeros((), dtype=torch.float32)
    assert torch.equal(torch.where(torch.isnan(got), zero, got), torch.where(torch.isnan(want), zero, want)), name


def _same(got, want):
    """Every field of a GrownSegments against the restatement's dict."""
    for name in INT_FIELDS:
        assert want[name].dtype == np.int32 and getattr(got, name).dtype == torch.int32, name
        assert torch.equal(getattr(got, name).cpu(), torch.from_numpy(want[name])), name
    assert {k: getattr(got, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert got.grid == want["grid"]
    for name in TABLES:
        if want.get(name) is None:
            assert getattr(got, name) is None, name
        else:
            _same_floats(getattr(got, name), want[name], name)
    for name in ("voxel_support", "voxel_ring"):
        if want.get(name) is None:
            assert getattr(got, name) is None, name
        else:
            assert getattr(got, name).dtype == torch.int32 and getattr(got, name).device == got.segments.device, name
            assert torch.equal(getattr(got, name).cpu(), torch.from_numpy(want[name])), name


def _check(name, scan, rings, connectivity, voxel=C.VOX, colour_tol=AC.TOL, min_points=2, normal_tol=None):
    base = _base(name, scan, voxel, colour_tol, connectivity, min_points, normal_tol)
    want = A.absorb(base, connectivity, rings)
    got = G.absorb_segments(scan, voxel=voxel, colour_tol=colour_tol, connectivity=connectivity, min_points=min_points,
                          normal_tol=normal_tol, absorb=rings)
    _same(got, want)
    return got, want


def _seg_at(got, coords, v):
    return int(got.segments[np.flatnonzero((coords == v).all(1))[0]])


# ---- 1. the crafted cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_a_round_reads_the_state_at_its_start(connectivity):
    """A f f f f B: the first round takes the two end voxels, the second splits the rest two and two.  Updating one table in
    place hands all four to one side."""
    scan, coords = _cached("chain", AC.chain_case)
    along = lambda got: [_seg_at(got, coords, (x, 0, 0)) for x in range(6)]
    assert along(_check("chain", scan, 0, connectivity)[0]) == [0, -1, -1, -1, -1, 1]
    got, _ = _check("chain", scan, 1, connectivity)
    assert along(got) == [0, 0, -1, -1, 1, 1] and got.segment_points.tolist() == [4, 4] and got.n_dropped_points == 2
    got, _ = _check("chain", scan, 2, connectivity)
    assert along(got) == [0, 0, 0, 1, 1, 1] and got.segment_points.tolist() == [5, 5] and got.n_dropped_points == 0
    assert got.voxel_ring.tolist() == [0, 1, 2, 2, 1, 0] and (got.n_absorbed_voxels, got.n_absorbed_points) == (4, 4)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_majority_decides_and_the_lower_root_wins_a_tie(connectivity):
    scan, coords = _cached("majority", AC.majority_case)
    got, want = _check("majority", scan, 1, connectivity, min_points=AC.MAJ_MIN)
    of = lambda v: _seg_at(got, coords, v)
    assert got.n_segments == 4 and got.n_absorbed_voxels == 2
    assert of(AC.MAJ_TIE) == of(AC.MAJ_TIE_LOW) < of(AC.MAJ_TIE_HIGH)
    assert of(AC.MAJ_TWO) == of(AC.MAJ_TWO_HIGH[0]) == of(AC.MAJ_TWO_HIGH[2]) > of(AC.MAJ_TWO_LOW)


def test_a_diagonal_neighbour_absorbs_with_26_and_not_with_6():
    scan, coords = _cached("diagonal", AC.diagonal_case)
    got, _ = _check("diagonal", scan, 3, 6)
    assert got.n_absorbed_voxels == 0 and all(_seg_at(got, coords, v) == -1 for v in AC.DIAG_FREE)
    got, _ = _check("diagonal", scan, 3, 26)
    assert got.n_absorbed_voxels == 2 and [_seg_at(got, coords, v) for v in AC.DIAG_FREE] == [0, 1]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_consecutive_keys_across_a_row_or_a_slab_are_no_neighbours(connectivity):
    """A free voxel at x = nx - 1 whose key + 1 is a kept voxel at x = 0 of the next row, the same the other way round and
    across two slabs: none of them is absorbed, whatever the ring count; the free voxel that has a neighbour is."""
    scan, coords = _cached("ends", AC.ends_case)
    for rings in (1, 64):
        got, want = _check("ends", scan, rings, connectivity)
        assert got.grid == AC.ENDS_GRID and got.n_segments == 5 and got.n_absorbed_voxels == 1 and got.n_dropped_points == 4
        assert all(_seg_at(got, coords, free) == -1 and _seg_at(got, coords, kept) >= 0 for free, kept in AC.ENDS_PAIRS)
        assert _seg_at(got, coords, AC.ENDS_TAKEN) == _seg_at(got, coords, AC.ENDS_TAKER)


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("rings", [1, 2, 5])
def test_every_face_edge_and_corner_of_a_full_grid(rings, connectivity):
    """12 x 11 x 10 voxels, all occupied; a quarter of them free, among them three corners of the grid."""
    scan, _ = _cached("full", AC.full_grid_case)
    got, want = _check("full", scan, rings, connectivity, min_points=AC.FULL_MIN)
    assert got.grid == (12, 11, 10) and got.n_voxels == 1320 and got.n_segments >= 2
    assert got.n_absorbed_voxels > 250 and 1 <= int(got.voxel_ring.max()) <= rings
    corner = got.voxel_ring[[0, 1319]].tolist()  # the voxels (0, 0, 0) and (11, 10, 9): free, with 3 or 7 neighbours
    assert all(r != 0 for r in corner) and want["voxel_ring"][[0, 1319]].tolist() == corner


@pytest.mark.parametrize("axis", [0, 2])
def test_an_axis_of_1024_voxels(axis):
    scan, _ = _cached(("strip", axis), lambda: AC.strip_case(axis))
    got, want = _check(("strip", axis), scan, 1, 6, voxel=0.05)
    assert got.grid == ((1024, 2, 1) if axis == 0 else (1, 2, 1024)) and got.n_voxels == 2048 and got.n_segments == 1
    assert got.n_absorbed_voxels == 1024 and got.segment_points.tolist() == [2048] and got.n_dropped_points == 0
    assert _check(("strip", axis), scan, 0, 6, voxel=0.05)[0].n_dropped_points == 1024


@pytest.mark.parametrize("connectivity", [6, 26])
def test_an_island_that_touches_nothing_kept_stays_free(connectivity):
    scan, coords = _cached("island", AC.island_case)
    for rings in (1, 3, 64):
        got, _ = _check("island", scan, rings, connectivity)
        assert got.n_absorbed_voxels == 1 and got.n_dropped_points == 3 and all(_seg_at(got, coords, v) == -1 for v in AC.ISLAND)
    # everything dropped: S = 0, nothing to be absorbed into
    got, _ = _check("island", scan, 64, connectivity, min_points=100)
    assert got.n_segments == 0 and (got.segments == -1).all() and (got.voxel_ring == -1).all() and got.voxel_ring.shape == (5,)
    assert got.n_absorbed_points == 0 and got.n_dropped_points == len(scan) and got.segment_points.shape == (0,)


@pytest.mark.parametrize("connectivity", [6, 26])
def test_many_owners_in_one_wave(connectivity):
    """130 kept voxels, a segment each, and 130 free ones above them: the free rows fill two waves of the end kernel with 64
    distinct owners each, every one of which gets its own points and nobody else's.  With 26 a free voxel has one neighbour
    in each of three segments and the smallest root wins."""
    scan, coords = _cached("comb", AC.comb_case)
    along = lambda got, y: [_seg_at(got, coords, (x, y, 0)) for x in range(AC.COMB_N)]
    got, _ = _check("comb", scan, 0, connectivity)
    assert got.n_segments == AC.COMB_N and along(got, 0) == list(range(AC.COMB_N)) and along(got, 1) == [-1] * AC.COMB_N
    got, _ = _check("comb", scan, 1, connectivity)
    owner, points = AC.comb_expected(connectivity)
    assert along(got, 0) == list(range(AC.COMB_N)) and along(got, 1) == owner and got.segment_points.tolist() == points
    assert (got.n_absorbed_voxels, got.n_absorbed_points, got.n_dropped_points) == (AC.COMB_N, AC.COMB_N, 0)


def test_64_rings_on_a_free_chain_of_70():
    scan, coords = _cached("open", AC.open_chain_case)
    got, _ = _check("open", scan, 64, 6)
    assert got.n_absorbed_voxels == 64 and got.n_dropped_points == 6 and got.segment_points.tolist() == [3 + 64]
    assert [_seg_at(got, coords, (x, 0, 0)) for x in (64, 65, 70)] == [0, -1, -1] and int(got.voxel_ring.max()) == 64
    got, _ = _check("open", scan, 63, 26)
    assert got.n_absorbed_voxels == 63


def test_more_rings_than_needed_give_the_bits_of_the_smallest_sufficient_count():
    scan, _ = _cached("chain", AC.chain_case)
    two = _check("chain", scan, 2, 6)[0]
    for rings in (3, 10, 64):
        more = _check("chain", scan, rings, 6)[0]
        assert all(np.array_equal(x, y) for x, y in zip(_fields(two), _fields(more)))
    scan, _ = _cached("full", AC.full_grid_case)
    enough = int(_check("full", scan, 64, 26, min_points=AC.FULL_MIN)[0].voxel_ring.max())
    assert 1 <= enough < 10
    a, b = (_check("full", scan, r, 26, min_points=AC.FULL_MIN)[0] for r in (enough, 64))
    assert all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(b)))


def test_absorbed_voxels_of_257_and_2600_points():
    scan, coords = _cached("big", AC.big_case)
    base = _check("big", scan, 0, 6, min_points=AC.BIG_MIN)[0]
    assert base.segment_points.tolist() == [3000] and base.n_dropped_points == 257 + 2600 + 2
    one = _check("big", scan, 1, 6, min_points=AC.BIG_MIN)[0]
    assert one.segment_points.tolist() == [3000 + 257 + 2] and (one.n_absorbed_voxels, one.n_absorbed_points) == (2, 259)
    two = _check("big", scan, 2, 6, min_points=AC.BIG_MIN)[0]
    assert two.segment_points.tolist() == [len(scan)] and (two.n_absorbed_voxels, two.n_absorbed_points) == (3, 2859)
    assert two.n_dropped_points == 0 and not two.segments.any()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_invalid_points_stay_out(connectivity):
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    bad = ~np.isfinite(scan[:, :3]).all(1)
    for rings in (1, 4):
        got, want = _check("invalid", scan, rings, connectivity, voxel=0.05, colour_tol=0.25, min_points=20)
        assert got.n_invalid == bad.sum() > 100 and (got.segments.cpu().numpy()[bad] == -1).all()
        assert got.n_absorbed_points > 100 and got.n_segments >= 2
    only_bad = np.full((300, 3), np.nan, f32)
    got, _ = _check("all-invalid", only_bad, 3, 6, colour_tol=None)
    assert got.n_voxels == 0 and got.voxel_ring.shape == (0,) and got.voxel_ring.dtype == torch.int32 and got.n_absorbed_voxels == 0
    assert _check("all-invalid", only_bad, 0, 6, colour_tol=None)[0].voxel_ring is None


# ---- 2. the other keywords --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("colour_tol", [None, 0.125])
def test_two_planes_get_their_edge_back(colour_tol, connectivity):
    """The fixture of the normal_tol tests with min_points = 100: 270 points in 90 voxels along the shared edge are dropped;
    one ring takes 180 of them back and leaves 30 voxels free, two rings take them all.  The planes keep their ids."""
    scan, coords = _cached("planes", NC.two_planes_case)
    kw = dict(voxel=0.05, colour_tol=colour_tol, min_points=100, normal_tol=10)
    zero, _ = _check("planes", scan, 0, connectivity, **kw)
    assert zero.n_segments == 2 and zero.n_dropped_points == 270 and zero.voxel_ring is None
    one, _ = _check("planes", scan, 1, connectivity, **kw)
    assert (one.n_segments, one.n_absorbed_points, one.n_absorbed_voxels, int((one.voxel_ring < 0).sum())) == (2, 180, 60, 30)
    two, _ = _check("planes", scan, 2, connectivity, **kw)
    assert (two.n_segments, two.n_absorbed_points, two.n_absorbed_voxels, int((two.voxel_ring < 0).sum())) == (2, 270, 90, 0)
    assert two.n_dropped_points == 0 and int(two.segment_points.sum()) == len(scan) and (two.segments >= 0).all()
    had = zero.segments >= 0
    assert torch.equal(two.segments[had], zero.segments[had]) and torch.equal(one.segments[had], zero.segments[had])


@pytest.mark.parametrize("connectivity", [6, 26])
def test_with_normal_tol_and_colour_tol_on_a_random_scan(connectivity):
    scan, _ = _cached(("random", 1), lambda: C.random_case(1))
    for rings in (1, 3):
        got, _ = _check(("random", 1), scan, rings, connectivity, voxel=0.05, colour_tol=0.5, min_points=15, normal_tol=30.0)
        assert got.n_absorbed_voxels > 50 and got.voxel_normals is not None and got.voxel_means is not None
    got, _ = _check(("random", 1), scan, 2, connectivity, voxel=0.05, colour_tol=None, min_points=15, normal_tol=30.0)
    assert got.n_absorbed_voxels > 50 and got.voxel_means is None


# ---- 3. promises ------------------------------------------------------------------------------------------------------------
def _fields(got):
    out = [getattr(got, k).cpu().numpy() for k in INT_FIELDS] + [[getattr(got, k) for k in COUNTS], list(got.grid)]
    out += [getattr(got, k).cpu().numpy() for k in ("voxel_support", "voxel_ring") if getattr(got, k) is not None]
    return out + [getattr(got, k).cpu().numpy().view(np.uint32) for k in TABLES if getattr(got, k) is not None]


RANDOM_KW = dict(voxel=0.05, colour_tol=0.25, connectivity=26, min_points=20)


def test_two_calls_give_the_same_bits():
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    dev = torch.from_numpy(scan).cuda()
    a = G.absorb_segments(dev, absorb=3, **RANDOM_KW)
    b = G.absorb_segments(dev, absorb=3, **RANDOM_KW)
    c = G.absorb_segments(scan, absorb=3, **RANDOM_KW)  # from the host
    d = G.absorb_segments(dev, normal_tol=30.0, absorb=3, **RANDOM_KW)
    e = G.absorb_segments(dev, normal_tol=30.0, absorb=3, **RANDOM_KW)
    assert a.n_absorbed_voxels > 50 and d.n_absorbed_voxels > 50
    for x, y in ((a, b), (a, c), (d, e)):
        assert all(np.array_equal(p, q) for p, q in zip(_fields(x), _fields(y)))


def test_absorb_0_launches_nothing_new_and_gives_the_bits_it_gave(monkeypatch):
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    with_rings = G.absorb_segments(scan, absorb=2, **RANDOM_KW)

    def never(*a, **k):
        raise AssertionError("the absorb entry point was called with absorb=0")
    monkeypatch.setattr(ops, "scene_grow_absorb", never)
    kw = dict(RANDOM_KW)
    conn = kw.pop("connectivity")
    got = G.absorb_segments(scan, connectivity=conn, absorb=0, **kw)
    plain = G.build_segments(scan, connectivity=conn, **kw)
    grown = G.grow_segments(scan, connectivity=conn, **kw)  # absorb_segments with absorb=0, under the signature it had
    assert got.voxel_ring is None and plain.voxel_ring is None and got.n_absorbed_voxels == got.n_absorbed_points == 0
    assert grown.voxel_ring is None and all(np.array_equal(p, q) for p, q in zip(_fields(got), _fields(grown)))
    _same(got, A.absorb(N.grow(scan, connectivity=conn, **kw), conn, 0))
    assert all(np.array_equal(p, q) for p, q in zip(_fields(got), _fields(plain)))
    with pytest.raises(AssertionError, match="absorb entry point"):
        G.absorb_segments(scan, connectivity=conn, absorb=1, **kw)
    # what absorb changes: -1s become ids, nothing else
    had = got.segments >= 0
    assert torch.equal(with_rings.segments[had], got.segments[had]) and with_rings.n_segments == got.n_segments
    assert torch.equal(with_rings.voxel_index, got.voxel_index) and (with_rings.segments[~had] >= 0).sum() == with_rings.n_absorbed_points


@pytest.mark.parametrize("normal_tol", [None, 30.0])
def test_ids_stay_counts_add_up_and_a_ring_more_changes_nothing_assigned(normal_tol):
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0)[0], 11))
    runs = {r: G.absorb_segments(scan, normal_tol=normal_tol, absorb=r, **RANDOM_KW) for r in (0, 1, 2, 3, 4)}
    zero = runs[0]
    assert zero.n_dropped_points > 500 and zero.n_segments >= 2
    for r in (1, 2, 3, 4):
        got, before = runs[r], runs[r - 1]
        had = zero.segments >= 0
        assert got.n_segments == zero.n_segments and got.n_components == zero.n_components
        assert torch.equal(got.segments[had], zero.segments[had])
        assert zero.n_dropped_points == got.n_dropped_points + got.n_absorbed_points
        assert int(got.segment_points.sum()) == int(zero.segment_points.sum()) + got.n_absorbed_points
        assert int((got.segments >= 0).sum()) == int(got.segment_points.sum())
        assert torch.equal(torch.bincount(got.segments[got.segments >= 0].long(), minlength=got.n_segments).int(), got.segment_points)
        assigned = before.segments >= 0
        assert torch.equal(got.segments[assigned], before.segments[assigned])  # everything assigned at R is unchanged at R + 1
        if before.voxel_ring is not None:
            taken = before.voxel_ring >= 0
            assert torch.equal(got.voxel_ring[taken], before.voxel_ring[taken])
        assert got.n_absorbed_voxels == int((got.voxel_ring > 0).sum()) >= before.n_absorbed_voxels
    assert runs[1].n_absorbed_voxels > 50 and runs[2].n_absorbed_voxels > runs[1].n_absorbed_voxels


def test_permuting_the_rows_of_the_scan_permutes_the_segments():
    """Without colour_tol and normal_tol nothing depends on the order of a voxel's points.  (Adjacency alone joins every
    pair of neighbours, so a dropped component has no kept neighbour: the rings find nothing, and must find nothing.)"""
    scan = _cached("invalid", lambda: C.with_invalid(C.random_case(0, occupancy=0.2)[0], 12))
    perm = np.random.RandomState(61).permutation(len(scan))
    kw = dict(voxel=0.05, connectivity=6, min_points=40, absorb=3)
    a, b = G.absorb_segments(scan, **kw), G.absorb_segments(np.ascontiguousarray(scan[perm]), **kw)
    assert a.n_dropped_points > 100 and a.n_segments >= 1 and a.n_absorbed_voxels == 0
    assert torch.equal(a.segments.cpu()[perm], b.segments.cpu()) and torch.equal(a.voxel_index.cpu()[perm], b.voxel_index.cpu())
    assert torch.equal(a.voxel_ring, b.voxel_ring) and torch.equal(a.segment_points, b.segment_points)
    _same(a, A.absorb(N.grow(scan, 0.05, None, 6, 40), 6, 3))


def test_pool_segments_takes_the_result_as_it_is():
    scan, _ = _cached("planes", NC.two_planes_case)
    M = len(scan)
    rs = np.random.RandomState(62)
    votes = rs.randint(0, 4, M).astype(np.int32)
    scores = (rs.randn(M, 5) * 3).astype(f32) * np.maximum(votes, 1)[:, None].astype(f32)
    labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)
    res = scene.SceneResult(torch.from_numpy(labels).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(votes).cuda(),
                            1, 1, int((labels == -1).sum()), 0)
    sg = G.absorb_segments(scan, min_points=100, normal_tol=10, absorb=2)
    want = A.absorb(_base("planes", scan, 0.05, None, 6, 100, 10), 6, 2)
    a = SS.pool_segments(res, sg.segments)
    b = SS.pool_segments(res, torch.from_numpy(want["segments"]))
    assert a.n_segments == b.n_segments == 2 and torch.equal(a.segment_points, sg.segment_points)
    assert int(a.segment_points.sum()) == M  # the edge is pooled with the planes: no point is left out
    for name in ("labels", "pooled", "segment_index", "segment_ids", "segment_members", "segment_labels"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.segment_scores.view(torch.int32), b.segment_scores.view(torch.int32))
    plain = SS.pool_segments(res, G.grow_segments(scan, min_points=100, normal_tol=10).segments)
    assert int(plain.segment_points.sum()) == M - 270


def test_the_learners_forward_the_keyword():
    scan, _ = _cached("planes", NC.two_planes_case)
    learner = fitted.FittedLearner.__new__(fitted.FittedLearner)  # the forwards need no model
    a = learner.absorb_segments(scan, min_points=100, normal_tol=10, absorb=2)
    b = G.absorb_segments(scan, min_points=100, normal_tol=10, absorb=2)
    assert a.n_absorbed_points == 270 and all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(b)))
    c = learner.absorb_segments(scan, 0.05, None, 6, 100, 10, 1)  # positional, absorb last
    assert c.n_absorbed_points == 180
