"""extract_objects ("Objects from a labelled scan", O1-O8), without a device: the numpy restatement
tests/scene_objects_ref.py against a breadth-first search over (class, cell) pairs, the bounds that O7 and O8 promise, the
room's five objects, every ValueError of the argument check, and the C ABI."""
import os
import sys
from collections import deque

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_grow_ref as R  # noqa: E402
import scene_objects_cases as OC  # noqa: E402
import scene_objects_ref as OR  # noqa: E402

from r3dfsseg_amd import _lib, ops, scene_objects as SO  # noqa: E402

f32 = np.float32
EPS32 = float(np.finfo(f32).eps)
_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _case(name):
    return _cached(("case", name), OC.CASES[name])


def _ref(name, connectivity, min_points=1, ignore=()):
    scan, labels, _, voxel = _case(name)
    return _cached(("ref", name, connectivity, min_points, tuple(ignore)),
                   lambda: OR.extract(scan, labels, voxel, connectivity, min_points, ignore))


def _bfs(scan, labels, voxel, connectivity):
    """Components of the (class, cell) pairs by a breadth-first search over a dense occupancy grid per class ->
    [(class, smallest cell key, sorted scan indices)], sorted by class, then key."""
    valid, _, coords, (nx, ny, nz) = R.voxels_of(scan, voxel)
    idx = np.flatnonzero(valid)
    out = []
    for l in sorted(set(int(v) for v in labels[idx] if v >= 0)):
        mine = labels[idx] == l
        occ = np.zeros((nz, ny, nx), bool)
        c = coords[mine]
        occ[c[:, 2], c[:, 1], c[:, 0]] = True
        comp = np.full((nz, ny, nx), -1, np.int64)
        n = 0
        for z, y, x in zip(*np.nonzero(occ)):
            if comp[z, y, x] >= 0:
                continue
            comp[z, y, x] = n
            todo = deque([(x, y, z)])
            while todo:
                ax, ay, az = todo.popleft()
                for dx, dy, dz in R.offsets(connectivity):
                    bx, by, bz = ax + dx, ay + dy, az + dz
                    if 0 <= bx < nx and 0 <= by < ny and 0 <= bz < nz and occ[bz, by, bx] and comp[bz, by, bx] < 0:
                        comp[bz, by, bx] = n
                        todo.append((bx, by, bz))
            n += 1
        of_point = comp[c[:, 2], c[:, 1], c[:, 0]]
        keys = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
        for k in range(n):
            out.append((l, int(keys[of_point == k].min()), sorted(idx[mine][of_point == k].tolist())))
    return sorted(out, key=lambda t: t[:2])


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_the_restatement_finds_the_components_of_a_breadth_first_search(name, connectivity):
    scan, labels, _, voxel = _case(name)
    want = _bfs(scan, labels, voxel, connectivity)
    got = _ref(name, connectivity)
    assert got["n_objects"] == got["n_components"] == len(want) and got["n_dropped_points"] == 0
    for s, (l, _, members) in enumerate(want):  # O6: numbered by ascending class, then smallest cell key
        assert got["object_labels"][s] == l and np.flatnonzero(got["objects"] == s).tolist() == members
        assert got["object_points"][s] == len(members)
        assert got["object_units"][s] == len(set(got["unit_index"][members].tolist()))
    assert np.all(np.diff(got["object_labels"]) >= 0)
    assert (labels[got["objects"] >= 0] == got["object_labels"][got["objects"][got["objects"] >= 0]]).all()


def test_the_cases_hold_what_they_are_meant_to():
    mixed = _ref("mixed", 26)
    assert mixed["n_objects"] == 2 and mixed["object_labels"].tolist() == list(OC.MIXED_CLASSES) and mixed["n_labels"] == 4
    assert mixed["object_units"].tolist() == [24, 24] and mixed["n_units"] == 48 and mixed["grid"] == (4, 3, 2)
    for conn in (6, 26):
        wrap = _ref("wrap", conn)
        assert wrap["grid"] == (5, 4, 3) and wrap["n_labels"] == 5
        keys = wrap["unit_keys"].tolist()
        for l in (2, 3):  # the last cell of class l and the first of class l + 1: consecutive keys, no neighbours
            a, b = keys.index(l * 60 + 59), keys.index((l + 1) * 60)
            assert b == a + 1 and wrap["unit_component"][a] != wrap["unit_component"][b]
        comp = {k % 60: c for k, c in zip(keys, wrap["unit_component"].tolist()) if k // 60 == 2}
        for a, b in OC.C.WRAP_PAIRS:  # row ends and slab ends within class 2
            ka, kb = (a[2] * 4 + a[1]) * 5 + a[0], (b[2] * 4 + b[1]) * 5 + b[0]
            assert kb == ka + 1 and comp[ka] != comp[kb]
        assert _ref("gap", conn)["n_objects"] == OC.GAP_OBJECTS[conn]
        snake = _ref("serpentine", conn)
        assert snake["n_units"] == 2177 > 2048 and snake["n_objects"] == 1
        checker = _ref("checker", conn)
        assert checker["n_units"] == checker["n_objects"] == 625 and (checker["unit_component"] == np.arange(625)).all()
        slab = _ref("slab", conn)
        assert slab["n_units"] == 300 > 256 and slab["n_objects"] == 1
    signs = _ref("signs", 26)
    assert signs["n_objects"] == 2
    bits = lambda v: int(np.asarray(v, f32).view(np.uint32))
    assert bits(signs["object_hi"][0, 0]) == 0 and bits(signs["object_lo"][0, 1]) == 0x80000000  # +0.0 above -0.0, -0.0 below
    assert bits(signs["object_hi"][1, 2]) == 0


def _total_order(v):
    return (float(v), 0 if np.signbit(v) else 1)  # -0.0 below +0.0


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_box_and_centroid_keep_what_o7_and_o8_promise(name):
    """The box is the minimum and maximum under the total order of O7.  The centroid lies within voxel / 512 of the float64
    mean, plus rounding: u + 0.5 is the sub-voxel coordinate to within half a step (1 / 512 of a voxel), and the subtraction,
    the division, the multiplication and the final rounding each add at most half an ulp of a value no larger than twice the
    largest coordinate -- 4 eps32 max|coordinate| in all.  The bound follows from O8, it is not measured."""
    scan, labels, _, voxel = _case(name)
    got = _ref(name, 26)
    big = float(np.abs(scan[np.isfinite(scan[:, :3]).all(1), :3]).max())
    bound = voxel / 512 + 4 * EPS32 * big
    assert got["n_objects"] >= 1
    for s in range(got["n_objects"]):
        pts = scan[got["objects"] == s, :3]
        assert len(pts) == got["object_points"][s]
        for a in range(3):
            lo, hi = min(pts[:, a], key=_total_order), max(pts[:, a], key=_total_order)
            assert got["object_lo"][s, a].view(np.uint32) == lo.view(np.uint32)
            assert got["object_hi"][s, a].view(np.uint32) == hi.view(np.uint32)
        err = np.abs(got["object_centroid"][s].astype(np.float64) - pts.astype(np.float64).mean(0))
        assert (err <= bound).all(), (s, err, bound)


def test_the_image_of_o7_keeps_the_order_of_the_floats():
    v = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], f32)
    im = OR.image(v)
    assert (np.diff(im.astype(np.int64)) > 0).all() and np.array_equal(OR.unimage(im).view(np.uint32), v.view(np.uint32))


def test_the_room_has_five_objects():
    """Floor, walls and three boxes.  min_points comes from the restatement's own sizes: the five largest objects, then a gap
    down to the specks that noise throws into a neighbouring cell's class."""
    sizes = np.sort(_ref("room", 6)["object_points"])[::-1]  # by faces alone: the list with the specks in it
    min_points, below, above = OC.room_min_points(sizes)
    assert len(sizes) >= 5 and above >= 20 * max(below, 1) and below < min_points <= above  # the gap min_points sits in
    for conn in (6, 26):
        got = _ref("room", conn, min_points)
        assert got["n_objects"] == 5 and got["object_labels"].tolist() == [0, 1, 2, 2, 2]
        assert got["n_dropped_points"] == len(_case("room")[0]) - got["object_points"].sum()


def test_ignore_and_bad_rows_in_the_restatement():
    scan, labels, _, voxel = _case("room")
    full, cut = _ref("room", 26), _ref("room", 26, ignore=(0,))
    assert cut["n_unlabelled"] == int((labels == 0).sum()) and 0 not in cut["object_labels"]
    assert cut["grid"] == full["grid"] and cut["n_objects"] == int((full["object_labels"] != 0).sum())
    bad_scan, bad_labels = OC.with_bad_rows(scan, labels, 31)
    got = OR.extract(bad_scan, bad_labels, voxel, 26)
    finite = np.isfinite(bad_scan[:, :3]).all(1)
    assert got["n_invalid"] == int((~finite).sum()) > 0 and got["n_unlabelled"] == int((finite & (bad_labels < 0)).sum()) > 0
    assert (got["objects"][~finite | (bad_labels < 0)] == -1).all() and (~finite & (bad_labels < 0)).any()
    none = OR.extract(scan, np.full(len(scan), -1, np.int64), voxel, 26)
    assert none["n_objects"] == none["n_units"] == none["n_labels"] == 0 and none["n_unlabelled"] == len(scan)
    assert none["grid"] == full["grid"] and (none["objects"] == -1).all()


# ---- the argument check ------------------------------------------------------------------------------------------------------
def _args(**over):
    a = dict(scan=np.zeros((10, 3), f32), labels=np.zeros(10, np.int64), voxel=0.05, connectivity=26, min_points=1, ignore=())
    a.update(over)
    return a


@pytest.mark.parametrize("over", [
    dict(scan=np.zeros((10, 2), f32)), dict(scan=np.zeros(10, f32)), dict(scan=np.zeros((0, 3), f32)), dict(scan=[[0.0, 0.0, 0.0]]),
    dict(scan=np.zeros((10, 3), np.float64)), dict(scan=torch.zeros(10, 3, dtype=torch.float16)),
    dict(labels=np.zeros(9, np.int64)), dict(labels=np.zeros((10, 1), np.int64)), dict(labels=[0] * 10),
    dict(labels=np.zeros(10, np.float32)), dict(labels=np.zeros(10, np.int16)), dict(labels=torch.zeros(10, dtype=torch.uint8)),
    dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(voxel=1e-60), dict(voxel="0.05"),
    dict(voxel=True), dict(voxel=None),
    dict(connectivity=18), dict(connectivity=6.0), dict(connectivity=True), dict(connectivity=None),
    dict(min_points=0), dict(min_points=-3), dict(min_points=1.0), dict(min_points=True),
    dict(ignore=(-1,)), dict(ignore=(1.0,)), dict(ignore=(True,)), dict(ignore=3), dict(ignore="0"), dict(ignore=(2 ** 63,)),
    dict(ignore=tuple(range(SO.MAX_IGNORE + 1))),
])
def test_bad_arguments_raise_before_a_device_is_needed(over):
    with pytest.raises(ValueError, match="extract_objects"):
        SO.check_object_args(**_args(**over))


def test_good_arguments_pass():
    scan, labels, voxel, ignore = SO.check_object_args(**_args(ignore=[3, 0, 3], labels=np.zeros(10, np.int32)))
    assert isinstance(scan, torch.Tensor) and labels.dtype == torch.int32 and voxel == f32(0.05) and ignore == (0, 3)
    assert SO.check_object_args(**_args(ignore=np.array([2, 1])))[3] == (1, 2)
    assert SO.check_object_args(**_args(ignore=tuple(range(SO.MAX_IGNORE))))[3] == tuple(range(SO.MAX_IGNORE))
    SO.check_object_args(**_args(scan=torch.zeros(10, 9), labels=torch.zeros(10, dtype=torch.int64)))


def test_the_key_range():
    assert SO.MAX_KEY == OR.MAX_KEY == 2 ** 31 - 1
    assert SO.check_key_range(1, (1024, 1024, 1024)) == 2 ** 30
    assert SO.check_key_range(2 ** 31 - 1, (1, 1, 1)) == 2 ** 31 - 1
    assert SO.check_key_range(7, (17, 19, 23)) == 7 * 17 * 19 * 23
    for n_labels, grid in ((2, (1024, 1024, 1024)), (2 ** 31, (1, 1, 1)), (1000, (200, 200, 60))):
        n_cells = grid[0] * grid[1] * grid[2]
        with pytest.raises(ValueError, match=r"%d labels .* %d cells .*larger voxel or renumber" % (n_labels, n_cells)):
            SO.check_key_range(n_labels, grid)


def test_the_abi_is_additive():
    assert _lib.ABI_VERSION == 6
    header = open(_lib.HEADER_PATH).read()
    assert "int r3d_abi_version(void); /* 6:" in header and _lib.load().r3d_abi_version() == 6
    names = ["r3d_scene_obj_%s" % n for n in ("ws_words", "bounds", "sort", "union", "components", "stats", "ids")]
    assert set(names) <= set(_lib.header_symbols()) and set(names) <= set(_lib._SIGS)
    assert [n for n in _lib.header_symbols() if n.startswith("r3d_scene_obj_")] == sorted(names)
    at = [header.index("int r3d_scene_obj_%s(" % n) for n in ("bounds", "sort", "union", "components", "stats", "ids")]
    assert at == sorted(at) and header.index("int r3d_scene_grow_ids(") < at[0]  # behind build_segments, in the call's order
    assert (ops.OBJ_R_NLABELS, ops.OBJ_R_NUNLABELLED, ops.OBJ_R_NOVER, ops.OBJ_R_NPOINTS) == (12, 13, 14, 15)
    assert ops.SCENE_OBJ_KEY == SO.MAX_KEY and ops.SCENE_OBJ_IGNORE == SO.MAX_IGNORE == 64


def test_the_library_exports_the_new_entry_points_and_refuses_bad_arguments():
    """No device is needed for an argument check: every entry point returns before it launches."""
    lib = _lib.load()
    M = 1000
    words = lib.r3d_scene_obj_ws_words(M)
    assert words == lib.r3d_scene_grow_ws_words(M) > 16  # one layout for both growers
    assert lib.r3d_scene_obj_ws_words(0) == -1 and lib.r3d_scene_obj_ws_words(2 ** 27 + 1) == -1
    one = 1  # a non-null pointer that is never read
    for rc in (lib.r3d_scene_obj_bounds(one, 3, M, one, 2, None, 0, one, words, None),           # labels64
               lib.r3d_scene_obj_bounds(one, 3, M, one, 0, None, 65, one, words, None),          # the ignore table
               lib.r3d_scene_obj_bounds(one, 3, M, one, 0, None, 0, one, words - 1, None),       # the workspace
               lib.r3d_scene_obj_sort(one, 3, M, one, 0, None, 0, 0.0, 0.0, 0.0, 0.05, 1024, 1024, 1024, 2, M, one, one, words,
                                      None),                                                      # the key range
               lib.r3d_scene_obj_union(M, 4, 4, 4, 1, 10, 18, one, words, None),                  # connectivity
               lib.r3d_scene_obj_components(M, 10, 0, one, words, None),                          # min_points
               lib.r3d_scene_obj_stats(one, 3, M, 0.0, 0.0, 0.0, 0.05, 4, 4, 4, 1, 10, 11, one, one, one, one, one, one, one, one,
                                       words, None),                                              # more objects than units
               lib.r3d_scene_obj_ids(M, M + 1, 0, one, one, one, words, None)):                   # more units than points
        assert rc != 0 and b"r3d_scene_obj_" in lib.r3d_last_error_string()
