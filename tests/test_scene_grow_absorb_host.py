"""absorb_segments (grow_segments with absorb, G6a), without a device: the numpy restatement tests/scene_grow_absorb_ref.py against a
breadth-first distance over a dense grid, the numbers of the two-planes fixture, what absorbing promises, the argument
checks, the signatures and the ABI."""
import collections
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_grow_absorb_cases as AC  # noqa: E402
import scene_grow_absorb_ref as A  # noqa: E402
import scene_grow_cases as C  # noqa: E402
import scene_grow_normals_cases as NC  # noqa: E402
import scene_grow_normals_ref as N  # noqa: E402
import scene_grow_ref as R  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, ops, scene_grow as G  # noqa: E402

f32 = np.float32


def dense_distance(base, connectivity):
    """The number of steps from every voxel to the nearest voxel of a kept component, through free voxels only, by a
    breadth-first search from all kept voxels at once over dense (nz, ny, nx) arrays; 0 for a kept voxel, -1 where no path
    leads to one.  base: the restatement's dict without absorb."""
    nx, ny, nz = base["grid"]
    keys = base["voxel_keys"]
    valid = base["voxel_index"] >= 0
    kept_voxel = np.zeros(len(keys), bool)
    kept_voxel[base["voxel_index"][valid]] = base["segments"][valid] >= 0
    dist = np.full((nz, ny, nx), -2, np.int64)  # -2: no voxel
    iz, iy, ix = keys // (nx * ny), (keys // nx) % ny, keys % nx
    dist[iz, iy, ix] = np.where(kept_voxel, 0, -1)
    queue = collections.deque(zip(iz[kept_voxel].tolist(), iy[kept_voxel].tolist(), ix[kept_voxel].tolist()))
    while queue:
        z, y, x = queue.popleft()
        for dx, dy, dz in R.offsets(connectivity):
            a, b, c = z + dz, y + dy, x + dx
            if 0 <= a < nz and 0 <= b < ny and 0 <= c < nx and dist[a, b, c] == -1:
                dist[a, b, c] = dist[z, y, x] + 1
                queue.append((a, b, c))
    return dist[iz, iy, ix]


CASES = {
    "chain": (lambda: AC.chain_case(), dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=AC.CHAIN_MIN)),
    "open chain": (lambda: AC.open_chain_case(), dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=2)),
    "majority": (AC.majority_case, dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=AC.MAJ_MIN)),
    "diagonal": (AC.diagonal_case, dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=2)),
    "ends": (AC.ends_case, dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=2)),
    "full grid": (AC.full_grid_case, dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=AC.FULL_MIN)),
    "island": (AC.island_case, dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=2)),
    "comb": (AC.comb_case, dict(voxel=C.VOX, colour_tol=AC.TOL, min_points=2)),
    "random": (lambda: C.random_case(1), dict(voxel=0.05, colour_tol=0.25, min_points=30)),
}


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", list(CASES))
def test_the_ring_is_the_breadth_first_distance_to_the_nearest_kept_voxel(name, connectivity):
    make, kw = CASES[name]
    scan = make()[0]
    base = R.grow(scan, connectivity=connectivity, **kw)
    dist = dense_distance(base, connectivity)
    prev = None
    for rings in (1, 2, 3, 7, 64):
        got = A.absorb(base, connectivity, rings)
        assert got["voxel_ring"].dtype == np.int32
        assert np.array_equal(got["voxel_ring"], np.where(dist <= rings, dist, -1)), (name, rings)
        _promises(base, got)
        if prev is not None:  # what one ring count assigned, a larger one leaves
            had = prev["segments"] >= 0
            assert np.array_equal(prev["segments"][had], got["segments"][had])
        prev = got
    assert (got["voxel_owner"][got["voxel_ring"] >= 0] >= 0).all() and (got["voxel_owner"][got["voxel_ring"] < 0] == -1).all()


def _promises(base, got):
    """S, the ids of absorb = 0 and the bookkeeping of the counts."""
    assert got["n_segments"] == base["n_segments"] and got["n_components"] == base["n_components"]
    had = base["segments"] >= 0
    assert np.array_equal(got["segments"][had], base["segments"][had])
    assert (got["segments"][base["voxel_index"] < 0] == -1).all()
    assert base["n_dropped_points"] == got["n_dropped_points"] + got["n_absorbed_points"]
    assert got["segment_points"].sum() == base["segment_points"].sum() + got["n_absorbed_points"]
    assert np.array_equal(np.bincount(got["segments"][got["segments"] >= 0], minlength=got["n_segments"]), got["segment_points"])
    assert (got["segments"] == -1).sum() == got["n_dropped_points"] + got["n_invalid"]
    assert got["n_absorbed_voxels"] == (got["voxel_ring"] > 0).sum()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_two_planes_get_their_edge_back(connectivity):
    """The fixture of the normal_tol tests: a floor and a wall of 30 x 30 voxels, three points per voxel.  With normal_tol the
    voxels along the shared edge are components of their own: 270 points in 90 voxels that min_points = 100 drops."""
    scan, coords = NC.two_planes_case()
    assert N.grow(scan, 0.05, None, connectivity, 1, normal_tol=10)["n_components"] == 14
    base = N.grow(scan, 0.05, None, connectivity, 100, normal_tol=10)
    assert base["n_segments"] == 2 and base["n_dropped_points"] == 270 and base["segment_points"].tolist() == [2520, 2520]
    zero = A.absorb(base, connectivity, 0)
    assert zero["voxel_ring"] is None and zero["n_absorbed_points"] == zero["n_absorbed_voxels"] == 0
    assert np.array_equal(zero["segments"], base["segments"]) and zero["n_dropped_points"] == 270
    one = A.absorb(base, connectivity, 1)
    assert (one["n_absorbed_points"], one["n_absorbed_voxels"], int((one["voxel_ring"] < 0).sum())) == (180, 60, 30)
    assert one["n_dropped_points"] == 90 and one["n_segments"] == 2
    two = A.absorb(base, connectivity, 2)
    assert (two["n_absorbed_points"], two["n_absorbed_voxels"], int((two["voxel_ring"] < 0).sum())) == (270, 90, 0)
    assert two["n_dropped_points"] == 0 and two["n_segments"] == 2 and two["segment_points"].sum() == len(scan)
    for got in (one, two):
        _promises(base, got)
    # the two planes keep their ids
    floor, wall = (coords[:, 2] == 0) & (coords[:, 0] >= 2), (coords[:, 0] == 0) & (coords[:, 2] >= 2)
    assert set(two["segments"][floor]) == set(base["segments"][floor]) and set(two["segments"][wall]) == set(base["segments"][wall])
    assert np.array_equal(A.absorb(base, connectivity, 64)["segments"], two["segments"])


def test_the_crafted_cases_of_the_restatement():
    scan, coords = AC.chain_case()
    base = R.grow(scan, C.VOX, AC.TOL, 6, AC.CHAIN_MIN)
    seg = lambda got, x: int(got["segments"][np.flatnonzero(coords[:, 0] == x)[0]])
    assert [seg(base, x) for x in range(6)] == [0, -1, -1, -1, -1, 1]
    assert [seg(A.absorb(base, 6, 1), x) for x in range(6)] == [0, 0, -1, -1, 1, 1]
    assert [seg(A.absorb(base, 6, 2), x) for x in range(6)] == [0, 0, 0, 1, 1, 1]  # in place: one side would take all four
    scan, coords = AC.majority_case()
    for conn in (6, 26):
        base = R.grow(scan, C.VOX, AC.TOL, conn, AC.MAJ_MIN)
        got = A.absorb(base, conn, 1)
        of = lambda v: int(got["segments"][np.flatnonzero((coords == v).all(1))[0]])
        assert base["n_segments"] == 4 and of(AC.MAJ_TIE) == of(AC.MAJ_TIE_LOW) < of(AC.MAJ_TIE_HIGH)
        assert of(AC.MAJ_TWO) == of(AC.MAJ_TWO_HIGH[0]) > of(AC.MAJ_TWO_LOW)
    scan, coords = AC.diagonal_case()
    for conn, taken in ((6, 0), (26, 2)):
        got = A.absorb(R.grow(scan, C.VOX, AC.TOL, conn, 2), conn, 5)
        assert got["n_absorbed_voxels"] == taken
    scan, coords = AC.ends_case()
    for conn in (6, 26):
        base = R.grow(scan, C.VOX, AC.TOL, conn, 2)
        got = A.absorb(base, conn, 64)
        assert base["grid"] == AC.ENDS_GRID and got["n_absorbed_voxels"] == 1 and got["n_dropped_points"] == 4
        keys = base["voxel_keys"].tolist()
        for free, kept in AC.ENDS_PAIRS:
            key = lambda v: (v[2] * 6 + v[1]) * 5 + v[0]
            assert abs(key(free) - key(kept)) == 1 and abs(keys.index(key(free)) - keys.index(key(kept))) == 1
            assert got["voxel_ring"][keys.index(key(free))] == -1
    scan, coords = AC.comb_case()  # 130 kept voxels, a segment each, and 130 free ones: 64 distinct owners in a wave of rows
    for conn in (6, 26):
        base = R.grow(scan, C.VOX, AC.TOL, conn, 2)
        seg = lambda got, y: [int(got["segments"][np.flatnonzero((coords == (x, y, 0)).all(1))[0]]) for x in range(AC.COMB_N)]
        assert base["n_segments"] == AC.COMB_N and seg(base, 0) == list(range(AC.COMB_N)) and seg(base, 1) == [-1] * AC.COMB_N
        got = A.absorb(base, conn, 1)
        owner, points = AC.comb_expected(conn)
        assert seg(got, 0) == list(range(AC.COMB_N)) and seg(got, 1) == owner and got["segment_points"].tolist() == points
        assert (got["n_absorbed_voxels"], got["n_absorbed_points"], got["n_dropped_points"]) == (AC.COMB_N, AC.COMB_N, 0)


def test_argument_errors_are_raised_without_a_device():
    ok = np.zeros((10, 3), f32)
    for r in (True, False, np.bool_(True), 1.0, 2.5, np.float32(1), "1", None, [1], (1,), 1j, -1, 65, 1000, np.int64(-3),
              float("nan")):
        with pytest.raises(ValueError, match="absorb .* must be an integer number of rings in 0 .. 64"):
            G.absorb_segments(ok, absorb=r)
        with pytest.raises(ValueError, match="absorb"):
            F.FittedLearner.__new__(F.FittedLearner).absorb_segments(ok, absorb=r)
        with pytest.raises(ValueError, match="absorb"):
            G.check_grow_args(ok, absorb=r)
    for r in (0, 1, 64, np.int32(3), np.int64(64)):
        G.check_grow_args(ok, absorb=r)
    with pytest.raises(ValueError, match="normal_tol"):  # the earlier checks still come first
        G.absorb_segments(ok, normal_tol=91, absorb=-1)


def test_signatures_and_abi():
    """absorb is the last keyword of absorb_segments; build_segments and grow_segments keep the parameters they had."""
    old = ["scan", "voxel", "colour_tol", "connectivity", "min_points"]
    assert list(inspect.signature(G.build_segments).parameters) == old
    assert list(inspect.signature(F.FittedLearner.build_segments).parameters) == ["self"] + old
    assert list(inspect.signature(G.grow_segments).parameters) == old + ["normal_tol"]
    assert list(inspect.signature(F.FittedLearner.grow_segments).parameters) == ["self"] + old + ["normal_tol"]
    assert list(inspect.signature(G.absorb_segments).parameters) == old + ["normal_tol", "absorb"]
    assert list(inspect.signature(G.check_grow_args).parameters) == old + ["normal_tol", "absorb"]
    assert list(inspect.signature(F.FittedLearner.absorb_segments).parameters) == ["self"] + old + ["normal_tol", "absorb"]
    from r3dfsseg_amd import mpti_learner, proto_contrast_learner, proto_learner
    for cls in (mpti_learner.MPTILearner_V3, proto_learner.ProtoLearner, proto_contrast_learner.ProtoContrastLearner):
        assert cls.absorb_segments is F.FittedLearner.absorb_segments
    for fn in (G.absorb_segments, F.FittedLearner.absorb_segments):
        defaults = {k: p.default for k, p in inspect.signature(fn).parameters.items() if k not in ("self", "scan")}
        assert defaults == dict(voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None, absorb=0)
    assert _lib.ABI_VERSION == 6 and G.MAX_RINGS == A.MAX_RINGS == 64
    assert (ops.GROW_R_ABSORBED_VOXELS, ops.GROW_R_ABSORBED_POINTS) == (12, 13) and ops.SCENE_GROW_REC == 16
    assert "r3d_scene_grow_absorb" in _lib.header_symbols()
    header = open(_lib.HEADER_PATH).read()
    at = [header.index("int r3d_scene_grow_%s(" % n) for n in ("components", "absorb", "ids")]  # the prototypes, in this order
    assert at == sorted(at)
    at = [header.index(" *   r3d_scene_grow_%s " % n) for n in ("components", "absorb", "ids")]  # and the table's rows
    assert at == sorted(at)


def test_the_entry_point_is_bound_and_checks_its_arguments():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    M = 1000
    words = lib.r3d_scene_grow_ws_words(M)
    ab = lib.r3d_scene_grow_absorb
    assert ab(M, 4, 4, 4, 10, 6, 1, None, p, words, None) != 0 and "null pointer (voxel_ring)" in err()
    assert ab(M, 4, 4, 4, 10, 6, 1, p, None, words, None) != 0 and "null pointer (ws)" in err()
    assert ab(M, 4, 4, 4, 10, 6, 1, p, p, words - 1, None) != 0 and "workspace of" in err()
    assert ab(M, 4, 4, 4, 10, 18, 1, p, p, words, None) != 0 and "connectivity 18" in err()
    assert ab(M, 4, 4, 4, 10, 6, 0, p, p, words, None) != 0 and "0 rings" in err()
    assert ab(M, 4, 4, 4, 10, 6, 65, p, p, words, None) != 0 and "65 rings" in err()
    assert ab(M, 4, 4, 4, 0, 6, 1, p, p, words, None) != 0 and "0 voxels" in err()
    assert ab(M, 4, 4, 4, M + 1, 6, 1, p, p, words, None) != 0 and "voxels of" in err()
    assert ab(M, 4, 1025, 4, 10, 6, 1, p, p, words, None) != 0 and "4 x 1025 x 4" in err()
    assert ab(0, 4, 4, 4, 10, 6, 1, p, p, words, None) != 0 and "M 0" in err()
    assert lib.r3d_scene_grow_ws_words(M) == words  # the workspace is the one it was
