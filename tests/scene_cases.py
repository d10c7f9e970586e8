"""Seeded scans for the predict_scene tests, and their numpy plans (tests/scene_ref.py), built once per session."""
import numpy as np

from scene_ref import RefPlan

f32 = np.float32
SMALL = dict(N=256, stride=0.5, min_points=100)
# points per cell of the small scan, row cy = 0..3, column cx = 0..5 (column 5 and row 3 end at the maximum point)
SMALL_CELLS = [[256, 0, 30, 20, 601, 1],
               [0, 0, 10, 196, 150, 0],
               [257, 0, 20, 60, 100, 0],
               [50, 120, 35, 141, 80, 1]]
FLAT_Z = f32(1.25)  # every point of cell (0, 0) -- which is all of block 0 for r = 1 and r = 2 -- has this z

_cache = {}


def _cell(v, v0, s):
    return int(np.floor((f32(v) - f32(v0)) / f32(s)))


def _at_least(v0, want, s, cell):
    """The fp32 number nearest v0 + want whose cell is `cell` (steps up by ulps if the rounding fell short)."""
    v = f32(f32(v0) + f32(want))
    while _cell(v, v0, s) < cell:
        v = np.nextafter(v, f32(np.inf), dtype=f32)
    assert _cell(v, v0, s) == cell
    return v


def small_scan():
    """(scan (M, 6) float32, info): ~2100 points on a 2.5 m x 1.7 m footprint at origin (-12.3, 40.7), stride 0.5; with
    points exactly on cell boundaries (the maximum point among them), exact duplicates, three non-finite points, empty
    cells, a flat block, and the block sizes the chunk rule branches on -- asserted below for r = 1 and r = 2."""
    if "small" in _cache:
        return _cache["small"]
    rs = np.random.RandomState(7)
    s, x0, y0 = f32(0.5), f32(-12.3), f32(40.7)
    xmax, ymax = _at_least(x0, 2.5, s, 5), _at_least(y0, 1.7, s, 3)
    row3 = lambda: f32(y0 + f32(1.5) + f32(rs.uniform(0.03, 0.17)))
    special = [(x0, y0), (xmax, ymax), (xmax, f32(y0 + f32(0.2)))]               # the corners, one more maximum-x point
    special += [(f32(x0 + f32(0.5 * k)), row3()) for k in (1, 2, 3, 4) for _ in range(3)]  # on x boundaries, in row 3
    special += [(f32(x0 + f32(2.0) + f32(rs.uniform(0.05, 0.45))), f32(y0 + f32(0.5 * k))) for k in (1, 2, 3) for _ in range(3)]
    on_boundary = len(special) - 1
    want = np.array(SMALL_CELLS)
    have = np.zeros_like(want)
    for x, y in special:
        have[_cell(y, y0, s), _cell(x, x0, s)] += 1
    assert (have <= want).all(), (have, want)
    pts = [(x, y, f32(rs.uniform(0, 3))) for x, y in special]
    n_dup = 0
    for cy in range(4):
        for cx in range(6):
            fill = []
            for _ in range(want[cy, cx] - have[cy, cx]):
                hi = 0.17 if cy == 3 else 0.45
                fill.append((f32(x0 + f32(0.5 * cx) + f32(rs.uniform(0.05, 0.45))), f32(y0 + f32(0.5 * cy) + f32(rs.uniform(0.03, hi))),
                             f32(rs.uniform(0, 3))))
            if len(fill) >= 100:  # exact duplicates: five points of the cell written over five others
                for a, b in zip(range(0, 5), range(50, 55)):
                    fill[b] = fill[a]
                n_dup += 5
            pts += fill
    xyz = np.array(pts, f32)
    in_flat = np.array([_cell(p[0], x0, s) == 0 and _cell(p[1], y0, s) == 0 for p in xyz])
    xyz[in_flat, 2] = FLAT_Z
    bad = np.array([[np.nan, y0 + 0.3, 1.0], [x0 + 0.3, np.inf, 1.0], [x0 + 0.3, y0 + 0.3, -np.inf]], f32)
    xyz = np.concatenate([xyz, bad])
    rgb = rs.randint(0, 256, (xyz.shape[0], 3)).astype(f32)
    scan = np.concatenate([xyz, rgb], 1)[rs.permutation(xyz.shape[0])]
    info = dict(on_boundary=on_boundary, n_dup=n_dup, n_bad=3, origin=(x0, y0))
    # the generator's promises, checked on the restated plan
    N, mp = SMALL["N"], SMALL["min_points"]
    for r in (1, 2):
        p = small_plan(r, scan)
        assert (p.ncx, p.ncy) == (6, 4) and p.x0 == x0 and p.y0 == y0 and p.xmax == xmax and p.ymax == ymax
        assert int((~p.valid).sum()) == 3 and (np.diff(p.cell_start) == want.reshape(-1)).all()
        assert (np.diff(p.cell_start) == 0).any()
        n = p.block_points
        nc = np.maximum(-(-n // N), 1)
        assert (n < mp).any() and ((n >= mp) & (n < N)).any() and (n == N).any() and (n == N + 1).any()
        assert ((n > 2 * N) & (n % nc != 0)).any()
        flat = p.block_list[0]
        assert len(flat) == 256 and (scan[flat, 2] == FLAT_Z).all()
    assert len(np.unique(scan[np.isfinite(scan).all(1)][:, :3], axis=0)) <= scan.shape[0] - 3 - n_dup
    _cache["small"] = (scan, info)
    return _cache["small"]


def small_plan(r, scan=None):
    key = ("small_plan", r)
    if key not in _cache:
        scan = small_scan()[0] if scan is None else scan
        _cache[key] = RefPlan(scan, SMALL["N"], block_size=0.5 * r, stride=0.5, min_points=SMALL["min_points"])
    return _cache[key]


MEDIUM = dict(N=256, stride=0.25, min_points=100, M=70001)


def medium_scan():
    """70 001 points (35 sort tiles) on 6 m x 5 m, stride 0.25: 24 x 20 = 480 cells, so two radix passes."""
    if "medium" not in _cache:
        rs = np.random.RandomState(3)
        M = MEDIUM["M"]
        xyz = rs.uniform(0, 1, (M, 3)).astype(f32) * np.array([5.999, 4.999, 3.0], f32) + np.array([3.1, -7.9, 0.0], f32)
        xyz[rs.randint(0, M, 5), rs.randint(0, 3, 5)] = np.nan
        _cache["medium"] = np.concatenate([xyz, rs.randint(0, 256, (M, 3)).astype(f32)], 1)
    return _cache["medium"]


def medium_plan(r):
    key = ("medium_plan", r)
    if key not in _cache:
        _cache[key] = RefPlan(medium_scan(), MEDIUM["N"], block_size=0.25 * r, stride=0.25, min_points=MEDIUM["min_points"])
        assert _cache[key].n_cells == 480
    return _cache[key]


WIDE = dict(N=4, stride=1.0, min_points=1, M=5000)


def wide_scan():
    """5 000 points whose extent makes exactly 256 x 256 = 65 536 cells: the key of the invalid points (65 536) needs a
    third 8-bit digit."""
    if "wide" not in _cache:
        rs = np.random.RandomState(11)
        xyz = rs.uniform(0, 1, (WIDE["M"], 3)).astype(f32) * np.array([255.0, 255.0, 3.0], f32)
        xyz[0, :2], xyz[1, :2] = (0.0, 0.0), (255.5, 255.5)
        xyz[7, 2] = np.inf
        _cache["wide"] = np.concatenate([xyz, rs.randint(0, 256, (WIDE["M"], 3)).astype(f32)], 1)
    return _cache["wide"]


def wide_plan():
    if "wide_plan" not in _cache:
        _cache["wide_plan"] = RefPlan(wide_scan(), WIDE["N"], block_size=1.0, stride=1.0, min_points=1)
        assert _cache["wide_plan"].n_cells == 65536
    return _cache["wide_plan"]
