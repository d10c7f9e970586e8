"""The scans of the normal_tol tests (host and GPU), built on tests/scene_grow_cases.py: integer voxel coordinates per point
and a position inside the voxel.  scan_of puts the lowest occupied layer of every axis at fraction 0, so a plane of voxels
that is the lowest layer of its axis is exactly flat."""
import numpy as np

import scene_grow_cases as C

f32 = np.float32
PLANE = 30


def two_planes_case(n=PLANE, points_per_voxel=3):
    """A floor z = 0 of n x n voxels and a wall x = 0 of n x n voxels that share the edge (0, y, 0), both exactly flat, the
    points at random places inside their planes; the floor is dark and the wall bright (0.25 and 0.75 in every channel)
    -> (scan, coords)."""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    floor = np.stack([x.ravel(), y.ravel(), np.zeros(n * n, np.int64)], 1)
    z, y = np.meshgrid(np.arange(1, n), np.arange(n), indexing="ij")
    wall = np.stack([np.zeros(len(z.ravel()), np.int64), y.ravel(), z.ravel()], 1)
    voxels = np.concatenate([floor, wall])
    colour = np.concatenate([np.full(len(floor), 0.25, f32), np.full(len(wall), 0.75, f32)])
    coords = np.repeat(voxels, points_per_voxel, 0)
    colours = np.repeat(colour, points_per_voxel)[:, None] * np.ones(3, f32)
    rs = np.random.RandomState(21)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    perm = rs.permutation(len(coords))
    return C.scan_of(coords[perm], frac[perm], colours[perm], voxel=0.05), coords[perm]


# a lone voxel; a line of three (support 2, 3, 2); a flat patch of exactly four; an L of four (not flat)
SMALL_LONE = [(0, 0, 0)]
SMALL_LINE = [(4, 0, 0), (5, 0, 0), (6, 0, 0)]
SMALL_PATCH = [(0, 4, 2), (1, 4, 2), (0, 5, 2), (1, 5, 2)]
SMALL_BENT = [(5, 4, 0), (6, 4, 0), (5, 5, 0), (5, 4, 1)]


def small_case(points_per_voxel=4):
    """-> (scan, coords).  The points of the flat patch all lie at half the voxel's height."""
    voxels = np.array(SMALL_LONE + SMALL_LINE + SMALL_PATCH + SMALL_BENT, np.int64)
    coords = np.repeat(voxels, points_per_voxel, 0)
    rs = np.random.RandomState(22)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    frac[(coords[:, 2] == 2), 2] = 0.5
    perm = rs.permutation(len(coords))
    return C.scan_of(coords[perm], frac[perm]), coords[perm]


def occupancy_case(share, grid=(12, 11, 10), seed=23, voxel=C.VOX):
    """A grid with the given share of occupied voxels (1.0: every voxel, so every face, edge and corner of the grid and every
    pair of consecutive keys across two rows), 1 .. 5 points per voxel anywhere inside it -> (scan, coords)."""
    rs = np.random.RandomState(seed + int(share * 100))
    nx, ny, nz = grid
    occ = rs.rand(nz, ny, nx) < share
    occ[0, 0, 0] = occ[-1, -1, -1] = True
    iz, iy, ix = np.nonzero(occ)
    voxels = np.stack([ix, iy, iz], 1)
    coords = np.repeat(voxels, rs.randint(1, 6, len(voxels)), 0)
    frac = rs.uniform(0.02, 0.98, coords.shape)
    perm = rs.permutation(len(coords))
    return C.scan_of(coords[perm], frac[perm], voxel=voxel), coords[perm]


BIG_VOXELS = {(1, 1, 0): 257, (3, 1, 0): 2600}


def big_voxel_case(voxel=0.05):
    """A 5 x 3 x 1 patch; voxel (1, 1, 0) holds 257 points and (3, 1, 0) holds 2600, the others 2, at random places (no
    multiples of anything) -> (scan, coords).  The centroids of the two big voxels depend on the order of the additions."""
    rs = np.random.RandomState(24)
    voxels = [(x, y, 0) for y in range(3) for x in range(5)]
    coords = np.concatenate([np.repeat(np.array([v], np.int64), BIG_VOXELS.get(v, 2), 0) for v in voxels])
    frac = rs.uniform(0.02, 0.98, coords.shape)
    perm = rs.permutation(len(coords))
    return C.scan_of(coords[perm], frac[perm], voxel=voxel, origin=(17.3, -4.9, 2.1)), coords[perm]


def strip_case(axis, n=1024):
    """A flat strip n x 2 voxels long, n along `axis` (0: x, 2: z), one point per voxel -> (scan, coords)."""
    k = np.arange(n)
    a, b = np.concatenate([k, k]), np.concatenate([np.zeros(n, np.int64), np.ones(n, np.int64)])
    zero = np.zeros(2 * n, np.int64)
    coords = np.stack([a, b, zero] if axis == 0 else [zero, b, a], 1)
    rs = np.random.RandomState(25 + axis)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    perm = rs.permutation(len(coords))
    return C.scan_of(coords[perm], frac[perm], voxel=0.05), coords[perm]


# ---- hand-made normal tables for the union entry point: pairs of voxels along x, three voxels apart
ULP1 = np.nextafter(f32(1), f32(2))
COS2 = f32(0.5)  # 45 degrees: float32(cos(radians(45)) ** 2) is 0.5 exactly
PAIRS = [
    # (row a, row b, joined, what it shows); with a = (1, 0, 0) and b = (1, y, 0): dot^2 = 1 and (c2 la) lb = (1 + y^2) / 2
    ((1, 0, 0), (1, 1, 0), True, "dot^2 = 1 equals (0.5 * 1) * 2 exactly"),
    ((1, 0, 0), (1, ULP1, 0), False, "(0.5 * 1) * (2 + 2^-22) = 1 + 2^-23: one ulp above dot^2"),
    ((1, 0, 0), (-1, -1, 0), True, "opposite signs"),
    ((-1, 0, 0), (1, 1, 0), True, "opposite signs, the other row"),
    ((2.0 ** -20, 0, 0), (2.0 ** 15, 2.0 ** 15, 0), True, "lengths 2^-20 and 2^15.5: dot^2 = 2^-10 = (0.5 * 2^-40) * 2^31"),
    ((2.0 ** -20, 0, 0), (2.0 ** 15, 2.0 ** 15 * ULP1, 0), False, "the same lengths, one ulp below"),
    ((np.nan, 0, 0), (1, 0, 0), False, "a NaN in a row"),
    ((1, 0, 0), (1, np.nan, 0), False, "a NaN in the other row"),
    ((np.nan, np.nan, np.nan), (np.nan, np.nan, np.nan), False, "two voxels without a normal"),
    ((np.inf, 0, 0), (1, 0, 0), True, "an infinite row: inf >= inf"),
    ((np.inf, 0, 0), (0, 1, 0), False, "an infinite row: inf * 0 is a NaN"),
    ((0, 0, 0), (1, 0, 0), True, "a row of zeros: la = 0, the test reads 0 >= 0"),
    ((0, 0, 0), (0, 0, 0), True, "two rows of zeros"),
    ((1, 0, 0), (0, 1, 0), False, "perpendicular"),
]


def pairs_case():
    """-> (scan, coords, table (V, 3) float32 in voxel-row order, joined list): pair p is voxels (3 p, 0, 0) and (3 p + 1, 0, 0)."""
    voxels = np.array([(3 * p + h, 0, 0) for p in range(len(PAIRS)) for h in (0, 1)], np.int64)
    rs = np.random.RandomState(26)
    perm = rs.permutation(len(voxels))
    table = np.array([row for a, b, _, _ in PAIRS for row in (a, b)], f32)  # rows ascend with x, as the keys do
    return C.scan_of(voxels[perm]), voxels[perm], table, [j for _, _, j, _ in PAIRS]
