"""The scans of the build_segments tests (host and GPU): voxel grids with a known occupancy, turned into points.

A case is made of integer voxel coordinates (ix, iy, iz) per point and a position inside the voxel as a fraction of its
edge.  Along every axis the points of the lowest occupied layer sit at fraction 0, so that the per-axis minimum of the scan
is that layer's face and the voxel of a point is its coordinate less the lowest one; the crafted cases use an edge of 0.5
and fractions that are multiples of 1 / 8, so every coordinate is exact in float32."""
import numpy as np

import scene_segments_ref

f32 = np.float32
VOX = 0.5
ORIGIN = (1.0, -2.0, 0.5)


def scan_of(coords, frac=None, colours=None, voxel=VOX, origin=ORIGIN, top_face=False):
    """coords (n, 3) ints, one row per point; frac (n, 3) in [0, 1) or None (0.5); colours (n, 3) or None (zeros) -> scan
    (n, 6) float32.  The lowest layer of every axis gets fraction 0; with top_face the highest one too (its points then sit
    exactly on the face that decides the number of voxels)."""
    coords = np.asarray(coords, np.int64)
    n = len(coords)
    frac = np.full((n, 3), 0.5) if frac is None else np.array(frac, np.float64)
    for a in range(3):
        frac[coords[:, a] == coords[:, a].min(), a] = 0.0
        if top_face:
            frac[coords[:, a] == coords[:, a].max(), a] = 0.0
    scan = np.zeros((n, 6), f32)
    scan[:, :3] = (np.asarray(origin, np.float64) + (coords + frac) * float(voxel)).astype(f32)
    if colours is not None:
        scan[:, 3:6] = colours
    return scan


def shuffled_within(groups, rs):
    """groups (n,) ints -> a permutation of 0 .. n - 1 (new row -> old row) that mixes the groups at random and keeps the
    order of the rows inside every group."""
    n = len(groups)
    slots, dest = rs.permutation(n), np.empty(n, np.int64)
    for g in np.unique(groups):
        idx = np.flatnonzero(groups == g)
        dest[idx] = np.sort(slots[idx])
    perm = np.empty(n, np.int64)
    perm[dest] = np.arange(n)
    return perm


# ---- 1. rows and slabs whose keys are consecutive
WRAP_GRID = (5, 4, 3)
# (last voxel of an x-row, first of the next row) twice, (last voxel of a slab, first of the next slab), the grid's corner
WRAP_PAIRS = [((4, 0, 0), (0, 1, 0)), ((4, 1, 2), (0, 2, 2)), ((4, 3, 1), (0, 0, 2))]
WRAP_CORNER = (4, 3, 2)


def wrap_case(points_per_voxel=5):
    """-> (scan, coords): nx ny nz = 5 4 3; the pairs above have consecutive keys and are no neighbours; the points of the
    corner voxel (4, 3, 2) sit exactly at the maximum of all three axes."""
    voxels = [v for pair in WRAP_PAIRS for v in pair] + [WRAP_CORNER]
    coords = np.repeat(np.array(voxels, np.int64), points_per_voxel, 0)
    rs = np.random.RandomState(5)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    perm = rs.permutation(len(coords))
    return scan_of(coords[perm], frac[perm], top_face=True), coords[perm]


# ---- 2. long thin components
def serpentine_voxels():
    """Two one-voxel-wide serpentines in a 33 x 33 x 1 grid -> (A, B) lists of (ix, iy, 0).  A fills the lines y = 0, 2, ..,
    14 and B the lines y = 18, 20, .., 32, each joined at alternating ends, 272 and 273 voxels long; A ends in (0, 15), B in
    (1, 16): the two share a corner and no face.  (Two disjoint one-voxel-wide paths with a gap between their lines hold
    about 580 voxels of a 33 x 33 grid together.)"""
    def snake(y0):
        cells = []
        for r in range(8):
            y = y0 + 2 * r
            cells += [(x, y, 0) for x in range(33)]
            if r < 7:
                cells.append((32 if r % 2 == 0 else 0, y + 1, 0))
        return cells
    A = snake(0) + [(0, 15, 0)]
    B = snake(18) + [(1, 17, 0), (1, 16, 0)]
    return A, B


def serpentine_case(points_per_voxel=3):
    A, B = serpentine_voxels()
    coords = np.repeat(np.array(A + B, np.int64), points_per_voxel, 0)
    rs = np.random.RandomState(6)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    perm = rs.permutation(len(coords))
    return scan_of(coords[perm], frac[perm]), coords[perm]


# ---- 3. contention
def full_grid_case(without_plane=None):
    """64 x 64 x 16 voxels, one point each, in a shuffled order; without_plane: that iz is left empty."""
    iz, iy, ix = np.meshgrid(np.arange(16), np.arange(64), np.arange(64), indexing="ij")
    coords = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1)
    if without_plane is not None:
        coords = coords[coords[:, 2] != without_plane]
    rs = np.random.RandomState(7)
    coords = coords[rs.permutation(len(coords))]
    return scan_of(coords), coords


# ---- 4. colour
COLOUR_TOL = 0.5
# along a line of voxels: joined, joined, apart (0.75), joined, then a NaN voxel that joins neither side, joined
COLOUR_LINE = [0.0, 0.5, 1.0, 1.75, 2.25, np.nan, 2.25, 2.75]
COLOUR_LINE_PARTS = [[0, 1, 2], [3, 4], [5], [6, 7]]


def colour_line_case():
    """Three lines of eight voxels along x, at y = 0, 2, 4, one point per voxel; line c carries COLOUR_LINE in channel c and
    1.0 in the others -> (scan, coords).  With COLOUR_TOL a line falls into COLOUR_LINE_PARTS."""
    coords, colours = [], []
    for c in range(3):
        for x, v in enumerate(COLOUR_LINE):
            coords.append((x, 2 * c, 0))
            col = [1.0, 1.0, 1.0]
            col[c] = v
            colours.append(col)
    rs = np.random.RandomState(8)
    perm = rs.permutation(len(coords))
    return scan_of(np.array(coords)[perm], colours=np.array(colours, f32)[perm]), np.array(coords)[perm]


def cancelling_case(channel=0):
    """Voxel (0, 0, 0) holds 257 points and voxel (0, 2, 0) holds 2600, with scene_segments_ref.cancelling_rows in `channel`
    in scan order; each has one neighbour, (1, 0, 0) and (1, 2, 0), of one point whose colour is the big voxel's mean by G3.
    With colour_tol = 0 a pair is joined exactly when the device sums in that order.  -> (scan, coords, means (2,) float32)."""
    coords, colour, group, means = [], [], [], []
    for g, (y, n) in enumerate([(0, 257), (2, 2600)]):
        rows = scene_segments_ref.cancelling_rows(n)[:, 0]
        mean = scene_segments_ref.pool_rows(rows[:, None])[0] / f32(n)
        means.append(mean)
        coords += [(0, y, 0)] * n + [(1, y, 0)]
        colour += list(rows) + [mean]
        group += [g] * (n + 1)
    coords, colour, group = np.array(coords, np.int64), np.array(colour, f32), np.array(group)
    perm = shuffled_within(group, np.random.RandomState(9))
    colours = np.full((len(coords), 3), 2.0, f32)
    colours[:, channel] = colour
    rs = np.random.RandomState(10)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    return scan_of(coords[perm], frac[perm], colours[perm]), coords[perm], np.array(means, f32)


# ---- 5. random
def random_case(seed, grid=(8, 24, 24), occupancy=0.40, voxel=0.05):
    """An nx x ny x nz grid with the given occupancy, 1 .. 12 points per occupied voxel in a shuffled scan order; every
    colour channel of a voxel is one of five levels 0.25 apart, and its points carry it -> (scan, coords)."""
    rs = np.random.RandomState(seed)
    nx, ny, nz = grid
    occ = rs.rand(nz, ny, nx) < occupancy
    iz, iy, ix = np.nonzero(occ)
    voxels = np.stack([ix, iy, iz], 1)
    per_voxel = rs.randint(1, 13, len(voxels))
    coords = np.repeat(voxels, per_voxel, 0)
    colours = np.repeat((rs.randint(0, 5, voxels.shape) * 0.25).astype(f32), per_voxel, 0)
    perm = rs.permutation(len(coords))
    coords, colours = coords[perm], colours[perm]
    frac = rs.randint(1, 8, coords.shape) / 8.0
    return scan_of(coords, frac, colours, voxel=voxel), coords


def with_invalid(scan, seed, share=0.03):
    """A copy of scan with NaN, +inf and -inf written into x, y or z of about `share` of its rows."""
    rs = np.random.RandomState(seed)
    out = scan.copy()
    rows = np.flatnonzero(rs.rand(len(scan)) < share)
    out[rows, rs.randint(0, 3, len(rows))] = rs.choice(np.array([np.nan, np.inf, -np.inf], f32), len(rows))
    return out
