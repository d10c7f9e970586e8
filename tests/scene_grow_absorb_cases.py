"""The scans of the absorb tests (host and GPU), built on tests/scene_grow_cases.scan_of.

Adjacency alone joins a voxel to every neighbour, so a voxel next to a kept segment is free only when a test parted it from
that segment.  The crafted cases part by colour: a cell is (voxel, points, colour), the colour goes to all three channels, two
colours differ by at least 1, and every case is grown with colour_tol = TOL.  A free voxel is a component of its own with
fewer points than the case's min_points."""
import numpy as np

import scene_grow_cases as C
import scene_grow_normals_cases as NC

f32 = np.float32
TOL = 0.25


def cells_case(cells, seed, voxel=C.VOX, top_face=False):
    """cells: (ix, iy, iz), points, colour -> (scan, coords) in a shuffled scan order."""
    voxels = np.array([c for c, _, _ in cells], np.int64)
    points = np.array([n for _, n, _ in cells])
    coords = np.repeat(voxels, points, 0)
    colours = np.repeat(np.array([col for _, _, col in cells], f32), points)[:, None] * np.ones(3, f32)
    rs = np.random.RandomState(seed)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    perm = rs.permutation(len(coords))
    return C.scan_of(coords[perm], frac[perm], colours[perm], voxel=voxel, top_face=top_face), coords[perm]


def rows_of(coords, voxel_index, voxels):
    """The voxel rows of the given (ix, iy, iz)."""
    return [int(voxel_index[np.flatnonzero((coords == v).all(1))[0]]) for v in voxels]


# ---- 1. a chain: A f f f f B.  min_points 2
CHAIN_MIN = 2


def chain_case(n_free=4):
    """Kept A at x = 0 and kept B at x = n_free + 1 (3 points each), n_free free voxels of one point between them."""
    cells = [((0, 0, 0), 3, 0.0)] + [((x, 0, 0), 1, 10.0 + x) for x in range(1, n_free + 1)] + [((n_free + 1, 0, 0), 3, 5.0)]
    return cells_case(cells, 51)


def open_chain_case(n_free=70):
    """Kept A at x = 0, then n_free free voxels: a free chain longer than the 64 rings there are."""
    return cells_case([((0, 0, 0), 3, 0.0)] + [((x, 0, 0), 1, 10.0 + x) for x in range(1, n_free + 1)], 52)


# ---- 2. majority and tie.  min_points 2
MAJ_TIE, MAJ_TIE_LOW, MAJ_TIE_HIGH = (1, 0, 0), (0, 0, 0), (2, 0, 0)
MAJ_TWO, MAJ_TWO_LOW, MAJ_TWO_HIGH = (6, 0, 0), (5, 0, 0), [(7, 0, 0), (7, 1, 0), (6, 1, 0)]
MAJ_MIN = 2


def majority_case():
    """(1, 0, 0) is free between one voxel of each of two segments: the lower root wins the tie.  (6, 0, 0) is free with one
    neighbour of the lower root, (5, 0, 0), and two of the higher, (7, 0, 0) and (6, 1, 0), joined through (7, 1, 0): the
    higher root has the majority (three to one with connectivity 26)."""
    cells = [(MAJ_TIE_LOW, 2, 1.0), (MAJ_TIE, 1, 20.0), (MAJ_TIE_HIGH, 2, 2.0),
             (MAJ_TWO_LOW, 2, 3.0), (MAJ_TWO, 1, 21.0)] + [(v, 2, 4.0) for v in MAJ_TWO_HIGH]
    return cells_case(cells, 53)


# ---- 3. a diagonal neighbour.  min_points 2
DIAG_FREE = [(1, 1, 0), (4, 1, 1)]  # an edge neighbour of (0, 0, 0), a corner neighbour of (3, 0, 0)


def diagonal_case():
    return cells_case([((0, 0, 0), 2, 0.0), (DIAG_FREE[0], 1, 10.0), ((3, 0, 0), 2, 1.0), (DIAG_FREE[1], 1, 11.0)], 54)


# ---- 4. the ends of a row and of a slab: nx ny nz = 5 4 2.  min_points 2
ENDS_GRID = (5, 6, 4)
# (free voxel, kept voxel) with consecutive keys, (iz * 6 + iy) * 5 + ix, across the end of a row or of a slab: no neighbours.
# No kept voxel lies within one step of a free one on every axis, so none of the four is ever absorbed.
ENDS_PAIRS = [((4, 0, 0), (0, 1, 0)),   # keys 4, 5: the end of a row, the kept voxel behind
              ((0, 3, 0), (4, 2, 0)),   # keys 15, 14: the kept voxel in front
              ((4, 5, 0), (0, 0, 1)),   # keys 29, 30: the end of a slab
              ((0, 0, 3), (4, 5, 2))]   # keys 90, 89
ENDS_TAKEN, ENDS_TAKER = (2, 3, 2), (2, 4, 2)  # a free voxel that does have a kept neighbour


def ends_case():
    cells = [(k, 2, float(i)) for i, (_, k) in enumerate(ENDS_PAIRS)] + [(f, 1, 10.0 + i) for i, (f, _) in enumerate(ENDS_PAIRS)]
    return cells_case(cells + [(ENDS_TAKER, 2, 6.0), (ENDS_TAKEN, 1, 16.0)], 55, top_face=True)


# ---- 5. a full grid.  min_points 6
FULL_MIN = 6


def full_grid_case(share_free=0.25):
    """scene_grow_normals_cases.occupancy_case(1.0): 12 x 11 x 10 voxels, all occupied, 1 .. 5 points each.  Colours: 0 for
    x < 6 and 1 behind, but a quarter of the voxels, at random, get a colour of their own: components of one voxel with at
    most 5 points, on every face, edge and corner of the grid."""
    scan, coords = NC.occupancy_case(1.0)
    nx, ny, nz = 12, 11, 10
    rs = np.random.RandomState(56)
    own = rs.rand(nz, ny, nx) < share_free
    own[0, 0, 0] = own[-1, -1, -1] = own[0, -1, 0] = True
    key = (coords[:, 2] * ny + coords[:, 1]) * nx + coords[:, 0]
    colour = np.where(own[coords[:, 2], coords[:, 1], coords[:, 0]], 2.0 + key, (coords[:, 0] >= 6).astype(np.float64))
    scan[:, 3:6] = colour.astype(f32)[:, None]
    return scan, coords


# ---- 6. a strip of 1024 x 2 voxels.  min_points 2
def strip_case(axis):
    """scene_grow_normals_cases.strip_case: the line b = 0 has one colour (a segment of 1024 points), every voxel of the
    line b = 1 a colour of its own (1024 free voxels of one point)."""
    scan, coords = NC.strip_case(axis)
    along = coords[:, 0] if axis == 0 else coords[:, 2]
    scan[:, 3:6] = np.where(coords[:, 1] == 0, 0.0, 2.0 + along).astype(f32)[:, None]
    return scan, coords


# ---- 7. an island.  min_points 2
ISLAND = [(5, 0, 0), (6, 0, 0), (5, 1, 0)]


def island_case():
    """A kept voxel with one free neighbour, and three free voxels that touch each other and nothing else."""
    return cells_case([((0, 0, 0), 2, 0.0), ((1, 0, 0), 1, 10.0)] + [(v, 1, 20.0 + i) for i, v in enumerate(ISLAND)], 57)


# ---- 8. a comb: many owners in one wave.  min_points 2
COMB_N = 130


def comb_case():
    """Kept voxels (x, 0, 0) of 2 points and colour x, each a segment of its own, and free voxels (x, 1, 0) of 1 point,
    x = 0 .. 129: the 130 free rows follow the 130 kept ones in the table, so the two full waves of free rows hold 64
    distinct owners each."""
    cells = [((x, 0, 0), 2, float(x)) for x in range(COMB_N)] + [((x, 1, 0), 1, 200.0 + x) for x in range(COMB_N)]
    return cells_case(cells, 59)


def comb_expected(connectivity):
    """One ring -> (the segment of free voxel (x, 1, 0) for every x, segment_points).  6: the kept voxel below it.  26: the
    kept voxels at x - 1, x and x + 1 tie with one neighbour each, the smallest root wins."""
    if connectivity == 6:
        return list(range(COMB_N)), [3] * COMB_N
    return [max(x - 1, 0) for x in range(COMB_N)], [4] + [3] * (COMB_N - 2) + [2]


# ---- 9. big voxels.  min_points 2601
BIG_MIN = 2601


def big_case():
    """A kept voxel of 3000 points; free voxels of 257 and of 2600 points in a line behind it, and one of 2 points."""
    return cells_case([((0, 0, 0), 3000, 0.0), ((1, 0, 0), 257, 10.0), ((2, 0, 0), 2600, 11.0), ((0, 1, 0), 2, 12.0)], 58)
