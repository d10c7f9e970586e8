"""grow_segments (build_segments with normal_tol), without a device: the numpy restatement tests/scene_grow_normals_ref.py against float64
eigenvectors and against a breadth-first search over a dense grid, what it promises (the sign of a normal does not matter,
normal_tol=None is the restatement without normals), the argument checks, the threshold, the signatures and the ABI."""
import collections
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_grow_cases as C  # noqa: E402
import scene_grow_normals_cases as NC  # noqa: E402
import scene_grow_normals_ref as N  # noqa: E402
import scene_grow_ref as R  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene_grow as G, synthetic as S  # noqa: E402

f32 = np.float32
MIN_GAP = 0.05       # (l1 - l0) / trace of the matrices the accuracy bar is stated for
MAX_ANGLE = 0.01     # degrees


def _full(C6):
    M = np.zeros((len(C6), 3, 3))
    for (i, j), c in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), range(6)):
        M[:, i, j] = M[:, j, i] = C6[:, c]
    return M


def test_the_normal_lies_within_a_hundredth_of_a_degree_of_the_smallest_eigenvector():
    """20 000 seeded positive semi-definite matrices Q diag(l) Q^T at scales 2^-40 .. 2^20, with eigenvalues drawn so that
    the gap (l1 - l0) / trace is at least 0.06, rounded to float32; the gap condition of the bar, (l1 - l0) / trace >= 0.05,
    is asserted on the float64 eigenvalues of every float32 matrix the test uses.  The reference is numpy.linalg.eigh in
    float64 on the same float32 matrix."""
    rng = np.random.default_rng(0)
    n = 20000
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    l2 = rng.uniform(0.2, 1.0, n)
    l1 = rng.uniform(0.1, 1.0, n) * l2
    l0 = rng.uniform(0.0, 1.0, n) * (0.94 * l1 - 0.06 * l2) / 1.06  # (l1 - l0) >= 0.06 (l0 + l1 + l2)
    lam = np.stack([l0, l1, l2], 1) * np.exp2(rng.integers(-40, 21, n))[:, None]
    Cm = np.einsum("nij,nj,nkj->nik", Q, lam, Q)
    C6 = np.stack([Cm[:, 0, 0], Cm[:, 0, 1], Cm[:, 0, 2], Cm[:, 1, 1], Cm[:, 1, 2], Cm[:, 2, 2]], 1).astype(f32)
    w, v = np.linalg.eigh(_full(C6.astype(np.float64)))
    gap = (w[:, 1] - w[:, 0]) / w.sum(1)
    assert (gap >= MIN_GAP).all()
    got, ok = N.normals_of_cov(C6)
    assert ok.all() and got.dtype == f32 and not np.isnan(got).any()
    assert (got.max(1) == 1).all()  # the row of the largest diagonal entry: that entry is 1 after the last rescaling
    g = got.astype(np.float64)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    angle = np.degrees(np.arccos(np.clip(np.abs((g * v[:, :, 0]).sum(1)), 0, 1)))
    print("worst angle %.3g degrees at gap %.3g" % (angle.max(), gap[angle.argmax()]))
    assert angle.max() <= MAX_ANGLE


def test_matrices_without_a_normal():
    bad = np.array([[0, 0, 0, 0, 0, 0], [1, 0, 0, np.inf, 0, 1], [1, np.nan, 0, 1, 0, 1], [-1, 0, 0, -1, 0, -1],
                    [1, 0, 0, 1, -np.inf, 1]], f32)
    got, ok = N.normals_of_cov(bad)
    assert not ok.any() and np.isnan(got).all()
    got, ok = N.normals_of_cov(np.array([[1, 0, 0, 1, 0, 0], [0, 0, 0, 2, 0, 2], [3, 0, 0, 0, 0, 3], [1, 0, 0, 1, 0, 1]], f32))
    assert ok.all() and got.tolist() == [[0, 0, 1], [1, 0, 0], [0, 1, 0], [1, 0, 0]]  # flat in z, x, y; a ball: the lowest on a tie


def test_the_threshold_is_the_float32_of_the_float64_squared_cosine():
    for t in (0, 0.0, 1e-3, 5, 10.0, 30, 45, 60.0, 89.999, 90, np.float32(12.5), np.int64(7)):
        want = np.float32(np.cos(np.radians(np.float64(t))) ** 2)
        got = G.cos2_of(t)
        assert type(got) is np.float32 and got == want == N.cos2_of(t), t
    assert G.cos2_of(0) == 1 and G.cos2_of(45) == f32(0.5) and 0 < G.cos2_of(90) < 1e-30
    assert G.cos2_of(10.0) == f32(0.9698463103929542)


def test_argument_errors_are_raised_without_a_device():
    ok = np.zeros((10, 3), f32)
    for t in (True, False, np.bool_(True), "10", [10.0], (1,), 1j, float("nan"), float("inf"), -float("inf"), -0.001, 90.001,
              -1, 91, 180, np.float32("nan")):
        with pytest.raises(ValueError, match="normal_tol .* must be None or a finite real number of degrees in \\[0, 90\\]"):
            G.grow_segments(ok, normal_tol=t)
        with pytest.raises(ValueError, match="normal_tol"):
            F.FittedLearner.__new__(F.FittedLearner).grow_segments(ok, normal_tol=t)
    # the earlier checks still come first and need no colour for normal_tol
    with pytest.raises(ValueError, match="colour_tol 0.1 given, but a scan of 3 columns has no colour"):
        G.grow_segments(ok, colour_tol=0.1, normal_tol=10.0)
    for t in (0, 90, 10.0, np.float32(3.5), np.int32(4)):
        G.check_grow_args(ok, normal_tol=t)


def test_signatures_and_abi():
    """normal_tol is the last keyword of grow_segments; build_segments keeps the parameters it had and is grow_segments
    without it."""
    old = ["scan", "voxel", "colour_tol", "connectivity", "min_points"]
    assert list(inspect.signature(G.build_segments).parameters) == old
    assert list(inspect.signature(G.grow_segments).parameters) == old + ["normal_tol"]
    assert list(inspect.signature(F.FittedLearner.grow_segments).parameters) == ["self"] + old + ["normal_tol"]
    for fn in (G.grow_segments, F.FittedLearner.grow_segments):
        defaults = {k: p.default for k, p in inspect.signature(fn).parameters.items() if k not in ("self", "scan")}
        assert defaults == dict(voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None)
    from r3dfsseg_amd import mpti_learner, proto_contrast_learner, proto_learner
    for cls in (mpti_learner.MPTILearner_V3, proto_learner.ProtoLearner, proto_contrast_learner.ProtoContrastLearner):
        assert cls.grow_segments is F.FittedLearner.grow_segments
    assert _lib.ABI_VERSION == 6
    for name in ("r3d_scene_grow_centroids", "r3d_scene_grow_normals", "r3d_scene_grow_union_normals"):
        assert name in _lib.header_symbols()


def test_entry_points_check_their_arguments():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    M = 1000
    words = lib.r3d_scene_grow_ws_words(M)
    assert lib.r3d_scene_grow_centroids(None, 6, M, 0.0, 0.0, 0.0, 0.05, 4, 4, 4, 10, p, p, words, None) != 0 and "null pointer" in err()
    assert lib.r3d_scene_grow_centroids(p, 2, M, 0.0, 0.0, 0.0, 0.05, 4, 4, 4, 10, p, p, words, None) != 0 and "ld 2" in err()
    assert lib.r3d_scene_grow_centroids(p, 3, M, 0.0, 0.0, 0.0, 0.05, 4, 4, 4, 10, p, p, words - 1, None) != 0 and "workspace of" in err()
    assert lib.r3d_scene_grow_centroids(p, 3, M, 0.0, 0.0, 0.0, 0.0, 4, 4, 4, 10, p, p, words, None) != 0 and "voxel size" in err()
    assert lib.r3d_scene_grow_centroids(p, 3, M, 0.0, float("nan"), 0.0, 0.05, 4, 4, 4, 10, p, p, words, None) != 0 and "origin" in err()
    assert lib.r3d_scene_grow_centroids(p, 3, M, 0.0, 0.0, 0.0, 0.05, 4, 4, 4, 0, p, p, words, None) != 0 and "0 voxels" in err()
    assert lib.r3d_scene_grow_centroids(p, 3, M, 0.0, 0.0, 0.0, 0.05, 4, 1025, 4, 10, p, p, words, None) != 0 and "4 x 1025 x 4" in err()
    assert lib.r3d_scene_grow_normals(M, 4, 4, 4, 10, 0.05, p, p, None, p, words, None) != 0 and "null pointer" in err()
    assert lib.r3d_scene_grow_normals(M, 4, 4, 4, 10, 0.05, p, p, p, None, words, None) != 0 and "null pointer (ws)" in err()
    assert lib.r3d_scene_grow_normals(M, 4, 4, 4, 10, float("inf"), p, p, p, p, words, None) != 0 and "voxel size" in err()
    assert lib.r3d_scene_grow_normals(M, 4, 4, 4, M + 1, 0.05, p, p, p, p, words, None) != 0 and "voxels of" in err()
    assert lib.r3d_scene_grow_normals(M, 0, 4, 4, 10, 0.05, p, p, p, p, words, None) != 0 and "0 x 4 x 4 voxels" in err()
    un = lib.r3d_scene_grow_union_normals
    assert un(M, 4, 4, 4, 10, 6, None, 0.0, None, 0.5, p, words, None) != 0 and "null pointer (voxel_normal)" in err()
    assert un(M, 4, 4, 4, 10, 6, None, 0.0, p, 1.5, p, words, None) != 0 and "cos2 1.5" in err()
    assert un(M, 4, 4, 4, 10, 6, None, 0.0, p, -0.1, p, words, None) != 0 and "cos2" in err()
    assert un(M, 4, 4, 4, 10, 6, None, 0.0, p, float("nan"), p, words, None) != 0 and "cos2" in err()
    assert un(M, 4, 4, 4, 10, 18, None, 0.0, p, 0.5, p, words, None) != 0 and "r3d_scene_grow_union_normals: connectivity 18" in err()
    assert un(M, 4, 4, 4, 10, 6, p, -1.0, p, 0.5, p, words, None) != 0 and "colour_tol" in err()
    assert un(M, 4, 4, 4, 10, 6, None, 0.0, p, 0.5, p, words - 1, None) != 0 and "workspace of" in err()


# ---- the restatement against itself and against an independent definition ---------------------------------------------------
def test_normal_tol_none_is_the_restatement_without_normals():
    scan, _ = C.random_case(0)
    for tol, conn, mp in ((None, 6, 1), (0.5, 26, 3)):
        a, b = N.grow(scan, 0.05, tol, conn, mp), R.grow(scan, 0.05, tol, conn, mp)
        assert a["voxel_centroids"] is None and a["voxel_normals"] is None and a["voxel_support"] is None
        for k, v in b.items():
            assert np.array_equal(a[k], v, equal_nan=True) if isinstance(v, np.ndarray) else a[k] == v, k


def test_the_sign_of_a_normal_does_not_matter():
    scan, _ = C.random_case(1)
    a = N.grow(scan, 0.05, None, 26, 1, normal_tol=20.0)
    assert 50 < a["n_components"] < a["n_voxels"] and np.bincount(a["voxel_component"]).max() > 10
    rs = np.random.RandomState(31)
    n = a["voxel_normals"]
    sign = rs.choice(np.array([-1, 1], f32), len(n))[:, None]
    scale = np.exp2(rs.randint(-10, 11, len(n))).astype(f32)[:, None]  # a power of two: every product stays exact
    for table in (n * sign, -n, n * sign * scale):
        b = N.grow(scan, 0.05, None, 26, 1, normals=table, cos2=N.cos2_of(20.0))
        assert np.array_equal(a["segments"], b["segments"]) and np.array_equal(a["voxel_component"], b["voxel_component"])
    pair = rs.randn(1000, 2, 3).astype(f32)
    for c2 in (0.0, 0.5, N.cos2_of(10), 1.0):
        want = N.alike(pair[:, 0], pair[:, 1], c2)
        assert np.array_equal(N.alike(-pair[:, 0], pair[:, 1], c2), want) and np.array_equal(N.alike(pair[:, 1], -pair[:, 0], c2), want)
    assert 0 < N.alike(pair[:, 0], pair[:, 1], 0.5).sum() < 1000


def test_the_hand_made_pairs_join_as_stated():
    scan, coords, table, joined = NC.pairs_case()
    assert N.cos2_of(45) == NC.COS2
    got = N.alike(table[0::2], table[1::2], NC.COS2)
    assert got.tolist() == joined, [w for (_, _, _, w), g, j in zip(NC.PAIRS, got, joined) if g != j]
    # the two boundary pairs lie one ulp apart
    dd, rhs = f32(1), (NC.COS2 * f32(1)) * (f32(1) + NC.ULP1 * NC.ULP1)
    assert rhs == np.nextafter(dd, f32(2))
    out = N.grow(scan, C.VOX, None, 6, 1, normals=table, cos2=NC.COS2)
    assert out["n_voxels"] == 2 * len(joined) and out["n_components"] == 2 * len(joined) - sum(joined)
    assert (out["voxel_support"] == 2).all() and np.isnan(out["voxel_normals"]).all()  # the scan's own: two voxels, no normal


def dense_components(normals, vcoord, vpoints, grid, c2, connectivity, means=None, colour_tol=None):
    """Breadth-first search over dense (nz, ny, nx) arrays, voxels visited in ascending (iz, iy, ix) order, so that
    components appear in ascending root order.  The angle test is written out here once more, in float32 scalars.
    -> (component of every voxel row, sizes in points)."""
    nx, ny, nz = grid
    row = np.full((nz, ny, nx), -1, np.int64)
    row[vcoord[:, 2], vcoord[:, 1], vcoord[:, 0]] = np.arange(len(vcoord))
    comp = np.full(len(vcoord), -1, np.int64)
    sizes = []

    def joins(a, b):
        p, q = normals[a], normals[b]
        with np.errstate(all="ignore"):
            dot = f32(f32(p[0] * q[0]) + f32(p[1] * q[1])) + f32(p[2] * q[2])
            la = f32(f32(p[0] * p[0]) + f32(p[1] * p[1])) + f32(p[2] * p[2])
            lb = f32(f32(q[0] * q[0]) + f32(q[1] * q[1])) + f32(q[2] * q[2])
            if not f32(dot * dot) >= f32(f32(c2 * la) * lb):
                return False
            return means is None or bool((np.abs(means[a] - means[b]) <= f32(colour_tol)).all())

    offs = R.offsets(connectivity)
    for start in range(len(vcoord)):  # rows ascend with the key, that is with (iz, iy, ix)
        if comp[start] >= 0:
            continue
        c, n = len(sizes), 0
        comp[start] = c
        queue = collections.deque([start])
        while queue:
            a = queue.popleft()
            n += int(vpoints[a])
            ax, ay, az = vcoord[a]
            for dx, dy, dz in offs:
                bx, by, bz = ax + dx, ay + dy, az + dz
                if not (0 <= bx < nx and 0 <= by < ny and 0 <= bz < nz):
                    continue
                b = row[bz, by, bx]
                if b < 0 or comp[b] >= 0 or not joins(a, b):
                    continue
                comp[b] = c
                queue.append(b)
        sizes.append(n)
    return comp, np.array(sizes, np.int64)


def _against_dense(scan, normal_tol, colour_tol, connectivity, min_points=1, voxel=0.05):
    got = N.grow(scan, voxel, colour_tol, connectivity, min_points, normal_tol=normal_tol)
    comp, sizes = dense_components(got["voxel_normals"], got["voxel_coords"], got["voxel_points"], got["grid"],
                                   N.cos2_of(normal_tol), connectivity, got["voxel_means"], colour_tol)
    assert got["n_components"] == len(sizes)
    roots = np.unique(got["voxel_component"])
    assert np.array_equal(np.searchsorted(roots, got["voxel_component"]), comp)
    kept = sizes >= min_points
    assert np.array_equal(got["segment_points"], sizes[kept].astype(np.int32)) and got["n_dropped_points"] == sizes[~kept].sum()
    new_id = np.full(len(sizes), -1, np.int32)
    new_id[kept] = np.arange(kept.sum(), dtype=np.int32)
    valid = got["voxel_index"] >= 0
    assert np.array_equal(got["segments"][valid], new_id[comp[got["voxel_index"][valid]]]) and (got["segments"][~valid] == -1).all()
    return got


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_restatement_equals_a_breadth_first_search_over_its_normals(connectivity):
    scan, _ = C.random_case(0)
    a = _against_dense(scan, 10.0, None, connectivity)
    b = _against_dense(scan, 90.0, None, connectivity)
    c = _against_dense(C.with_invalid(scan, 11), 30.0, 0.5, connectivity, min_points=4)
    z = _against_dense(scan, 0.0, None, connectivity)
    assert z["n_components"] >= a["n_components"] > b["n_components"] > R.grow(scan, 0.05, None, connectivity)["n_components"]
    assert c["n_invalid"] > 100 and c["n_dropped_points"] > 0
    # normal_tol = 90 is not None: a voxel without a normal stays alone
    lone = np.isnan(b["voxel_normals"][:, 0])
    assert lone.any() and (np.bincount(b["voxel_component"], minlength=b["n_voxels"])[np.flatnonzero(lone)] == 1).all()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_two_planes_fall_apart(connectivity):
    scan, coords = NC.two_planes_case(12)
    got = _against_dense(scan, 10.0, None, connectivity)
    seg = got["segments"]
    floor, wall = (coords[:, 2] == 0) & (coords[:, 0] >= 2), (coords[:, 0] == 0) & (coords[:, 2] >= 2)
    assert len(set(seg[floor])) == 1 and len(set(seg[wall])) == 1 and seg[floor][0] != seg[wall][0]
    n = got["voxel_normals"][got["voxel_index"]]
    assert (n[floor] == [0, 0, 1]).all() and (n[wall] == [1, 0, 0]).all()  # exactly flat planes
    assert R.grow(scan, 0.05, None, connectivity)["n_components"] == 1  # adjacency alone: one segment


def test_small_cases_of_the_restatement():
    scan, coords = NC.small_case()
    got = N.grow(scan, C.VOX, None, 26, 1, normal_tol=10.0)
    row = lambda v: got["voxel_index"][np.flatnonzero((coords == v).all(1))[0]]
    sup, nrm, comp = got["voxel_support"], got["voxel_normals"], got["voxel_component"]
    assert sup[row(NC.SMALL_LONE[0])] == 1 and [sup[row(v)] for v in NC.SMALL_LINE] == [2, 3, 2]
    for v in NC.SMALL_LONE + NC.SMALL_LINE:
        assert np.isnan(nrm[row(v)]).all() and (comp == comp[row(v)]).sum() == 1
    assert all(sup[row(v)] == 4 for v in NC.SMALL_PATCH + NC.SMALL_BENT)
    assert all(nrm[row(v)].tolist() == [0, 0, 1] for v in NC.SMALL_PATCH) and len({comp[row(v)] for v in NC.SMALL_PATCH}) == 1
    assert not np.isnan(nrm[[row(v) for v in NC.SMALL_BENT]]).any()


def test_the_big_voxels_centroids_depend_on_the_summation_order():
    scan, coords = NC.big_voxel_case()
    got = N.grow(scan, 0.05, None, 6, 1, normal_tol=10.0)
    valid, v0, q, grid = R.voxels_of(scan, 0.05)
    assert grid == (5, 3, 1) and np.array_equal(q, coords)
    differs = {}
    for v, n in NC.BIG_VOXELS.items():
        rows = np.flatnonzero((coords == v).all(1))
        assert len(rows) == n
        r = got["voxel_index"][rows[0]]
        u = (scan[rows, :3] - v0) - np.array(v, f32) * f32(0.05)
        assert u.dtype == f32 and (u > -1e-6).all() and (u < 0.05 + 1e-6).all()
        exact = (u.astype(np.float64).sum(0) / n).astype(f32)
        running = np.zeros(3, f32)
        for x in u:
            running = running + x
        back = np.zeros(3, f32)
        for x in u[::-1]:
            back = back + x
        others = [exact, back / f32(n)] + ([running / f32(n)] if n > 257 else [])  # 257: one running sum IS the tiled sum
        differs[n] = [bool((o != got["voxel_centroids"][r]).any()) for o in others]
        assert np.allclose(got["voxel_centroids"][r], exact, rtol=0, atol=1e-6)
    assert all(differs[2600]) and any(differs[257]), differs


def test_make_room_is_seeded_and_made_of_surfaces():
    a, la = S.make_room(3, n_points=20000)
    b, lb = S.make_room(3, n_points=20000)
    c, _ = S.make_room(4, n_points=20000)
    assert torch.equal(a, b) and torch.equal(la, lb) and not torch.equal(a, c)
    assert a.shape == (20000, 6) and a.dtype == torch.float32 and la.dtype == torch.int64 and int(la.max()) == 4 + 5 * 3
    assert float(a[:, 3:].min()) >= 0 and float(a[:, 3:].max()) <= 255
    xyz = a[:, :3].numpy() - np.array([-12.3, 40.7, 0.5], f32)
    assert np.abs(xyz[la.numpy() == 0, 2]).max() < 0.02 and np.abs(xyz[la.numpy() == 1, 0]).max() < 0.02  # the floor, a wall
    got = N.grow(a.numpy(), 0.05, None, 26, 1, normal_tol=10.0)
    top = np.sort(got["segment_points"])[::-1]
    assert R.grow(a.numpy(), 0.05, None, 26)["segment_points"].max() > 0.99 * 20000  # adjacency alone: the room is one segment
    assert top[0] < 0.3 * 20000 and top[4] > 1000  # with normals: the floor and the four walls, apart
