"""The scans of the extract_objects tests (host and GPU), built on tests/scene_grow_cases.scan_of: integer cell coordinates per
point, a position inside the cell as a fraction of its edge, and a class per point.  The crafted cases use an edge of 0.5 and
fractions that are multiples of 1 / 8, so every coordinate is exact in float32.  A case is (scan (M, 6) float32, labels (M,)
int64, coords (M, 3) ints or None, voxel)."""
import numpy as np

import scene_grow_cases as C

f32 = np.float32


def _points(cells, labels, per_cell, seed, top_face=False):
    """cells (n, 3), labels (n,): per_cell points each, at random fractions, in a shuffled scan order."""
    coords = np.repeat(np.asarray(cells, np.int64), per_cell, 0)
    lab = np.repeat(np.asarray(labels, np.int64), per_cell)
    rs = np.random.RandomState(seed)
    frac = rs.randint(1, 8, coords.shape) / 8.0
    perm = rs.permutation(len(coords))
    return C.scan_of(coords[perm], frac[perm], top_face=top_face), lab[perm], coords[perm], C.VOX


# ---- mixed: two classes in the same cells
MIXED_CLASSES = (1, 3)  # classes 0 and 2 hold nothing


def mixed_case():
    """A block of 4 x 3 x 2 cells, every cell with 3 points of class 1 and 3 of class 3: two objects that share all cells."""
    cells = [(x, y, z) for z in range(2) for y in range(3) for x in range(4)]
    return _points(cells * 2, [MIXED_CLASSES[0]] * len(cells) + [MIXED_CLASSES[1]] * len(cells), 3, 21)


# ---- wrap: keys that are consecutive across a row end, a slab end and a class boundary
WRAP_CLASSES = {2: [v for pair in C.WRAP_PAIRS for v in pair] + [C.WRAP_CORNER],  # the last cell of class 2 ...
                3: [(0, 0, 0), (1, 0, 0), C.WRAP_CORNER],                          # ... the first and the last of class 3 ...
                4: [(0, 0, 0)]}                                                    # ... and the first of class 4 are occupied


def wrap_case():
    """The grid and the corner of scene_grow_cases.wrap_case (5 x 4 x 3, points exactly at the maximum of all three axes).
    Class 2 holds its row-end and slab-end pairs; the corner cell of class l and the first cell of class l + 1 have consecutive
    keys for l = 2 and 3 and are no neighbours."""
    cells = [v for l in sorted(WRAP_CLASSES) for v in WRAP_CLASSES[l]]
    labels = [l for l in sorted(WRAP_CLASSES) for _ in WRAP_CLASSES[l]]
    return _points(cells, labels, 4, 22, top_face=True)


# ---- gap: one empty cell between two blobs, an edge, a corner
def gap_case():
    """One class.  Two blobs of 2 x 2 x 2 cells with the cells x = 2 empty between them; two cells that share only an edge; two
    that share only a corner: 4 objects at connectivity 26, 6 at 6."""
    blob = [(x, y, z) for z in range(2) for y in range(2) for x in range(2)]
    cells = blob + [(x + 3, y, z) for x, y, z in blob] + [(0, 4, 0), (1, 5, 0)] + [(0, 8, 0), (1, 9, 1)]
    return _points(cells, [5] * len(cells), 3, 23)


GAP_OBJECTS = {26: 4, 6: 6}


# ---- serpentine: one long thin object
def serpentine_cells(width=65, lines=33):
    """A one-cell-wide path through a width x (2 lines - 1) x 1 grid: the lines y = 0, 2, .. joined at alternating ends."""
    cells = []
    for r in range(lines):
        cells += [(x, 2 * r, 0) for x in range(width)]
        if r < lines - 1:
            cells.append((width - 1 if r % 2 == 0 else 0, 2 * r + 1, 0))
    return cells


def serpentine_case():
    """65 * 33 + 32 = 2177 units of class 1 in one object: finds walk chains across workgroups."""
    cells = serpentine_cells()
    return _points(cells, [1] * len(cells), 2, 24)


# ---- checker and slab: 64 distinct objects in every wave of the stats kernel, and a single one
def checker_case():
    """25 x 25 x 1 cells, all occupied, class (ix % 2) + 2 (iy % 2): the cells of one class lie two apart, so each of the 625
    units is its own object at either connectivity, and after the sort every wave of 64 rows holds 64 distinct roots."""
    cells = [(x, y, 0) for y in range(25) for x in range(25)]
    return _points(cells, [(x % 2) + 2 * (y % 2) for x, y, _ in cells], 2, 25)


def slab_case():
    """20 x 15 x 1 cells of one class: one object of 300 units, its waves hold a single root."""
    cells = [(x, y, 0) for y in range(15) for x in range(20)]
    return _points(cells, [2] * len(cells), 3, 26)


# ---- signs: coordinates that straddle zero
def signs_case():
    """Object A (class 0): x in {-0.5, -0.25, -0.0, +0.0}, so its largest x is +0.0 beside a -0.0; y in {-0.0, +0.0, 0.25, 0.375},
    so its smallest y is -0.0 beside a +0.0; z in {-0.5, -0.0, +0.0, 0.25}.  Object B (class 1), apart from it: x in 2 .. 2.5,
    y in -1 .. -0.75, z in -0.25 .. +0.0 with +0.0 its largest.  Every combination is a point; voxel 0.5."""
    neg = f32(-0.0)
    A = [(x, y, z) for x in (f32(-0.5), f32(-0.25), neg, f32(0)) for y in (neg, f32(0), f32(0.25), f32(0.375))
         for z in (f32(-0.5), neg, f32(0), f32(0.25))]
    B = [(x, y, z) for x in (f32(2), f32(2.25), f32(2.5)) for y in (f32(-1), f32(-0.75)) for z in (f32(-0.25), neg, f32(0))]
    scan = np.zeros((len(A) + len(B), 6), f32)
    scan[:, :3] = np.array(A + B, f32)
    labels = np.array([0] * len(A) + [1] * len(B), np.int64)
    perm = np.random.RandomState(27).permutation(len(scan))
    return scan[perm], labels[perm], None, 0.5


# ---- room: surfaces of synthetic.make_room
ROOM_VOXEL = 0.1


def labels_of_surface(surface):
    """make_room's surface column -> class 0 the floor, 1 the four walls, 2 the boxes."""
    surface = np.asarray(surface)
    return np.where(surface == 0, 0, np.where(surface <= 4, 1, 2)).astype(np.int64)


def room_case(n_points=20000, extent=(4.0, 3.0, 2.5)):
    from r3dfsseg_amd import synthetic
    scan, surface = synthetic.make_room(seed=0, n_points=n_points, extent=extent)
    return scan.numpy(), labels_of_surface(surface.numpy()), None, ROOM_VOXEL


def room_min_points(sizes):
    """sizes: the object sizes of the room at min_points = 1 -> (min_points, below, above): the five largest objects are
    the floor, the walls and the three boxes; min_points sits in the middle of the gap between the fifth and the sixth size."""
    sizes = np.sort(np.asarray(sizes))[::-1]
    above, below = int(sizes[4]), int(sizes[5]) if len(sizes) > 5 else 0
    return (above + below + 1) // 2, below, above


CASES = {"mixed": mixed_case, "wrap": wrap_case, "gap": gap_case, "serpentine": serpentine_case, "checker": checker_case,
         "slab": slab_case, "signs": signs_case, "room": room_case}


def with_bad_rows(scan, labels, seed):
    """A copy with non-finite coordinates in about 3 % of the rows (scene_grow_cases.with_invalid) and a negative label in
    about 5 % -- some rows get both."""
    out = C.with_invalid(scan, seed)
    rs = np.random.RandomState(seed + 1)
    lab = labels.copy()
    lab[rs.rand(len(lab)) < 0.05] = -1 - rs.randint(0, 3)
    return out, lab
