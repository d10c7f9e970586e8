"""extract_objects on the device (r3dfsseg_amd/scene_objects.py, csrc/scene_objects.hip) against the numpy restatement
tests/scene_objects_ref.py (which tests/test_scene_objects_host.py checks against a breadth-first search).

Every comparison is on integers, and bit for bit on the boxes and the centroids: the definition ("Objects from
a labelled scan") fixes every operation and its order, so no tolerance is used in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_grow_cases as C  # noqa: E402
import scene_objects_cases as OC  # noqa: E402
import scene_objects_ref as OR  # noqa: E402
import scene_segments_ref  # noqa: E402

from r3dfsseg_amd import fitted, ops, scene, scene_grow as G, scene_objects as SO, scene_segments as SS  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
INT_FIELDS = (("objects", np.int32), ("unit_index", np.int32), ("object_labels", np.int64), ("object_points", np.int32),
              ("object_units", np.int32))
FLOAT_FIELDS = ("object_lo", "object_hi", "object_centroid")
COUNTS = ("n_objects", "n_units", "n_components", "n_dropped_points", "n_unlabelled", "n_invalid", "n_labels")
_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _case(name):
    return _cached(("case", name), OC.CASES[name])


def _want(name, scan, labels, voxel, connectivity, min_points=1, ignore=()):
    """The restatement of a named scan, computed once."""
    return _cached(("ref", name, voxel, connectivity, min_points, tuple(ignore)),
                   lambda: OR.extract(scan, labels, voxel, connectivity, min_points, ignore))


def _same(got, want):
    """Every field of a SceneObjects against the restatement's dict."""
    for name, dtype in INT_FIELDS:
        a = getattr(got, name).cpu().numpy()
        assert a.dtype == want[name].dtype == dtype and np.array_equal(a, want[name]), name
    assert {k: getattr(got, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert got.grid == want["grid"]
    for name in FLOAT_FIELDS:
        a, b = getattr(got, name).cpu().numpy(), want[name]
        assert a.shape == b.shape == (want["n_objects"], 3) and a.dtype == b.dtype == f32, name
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def _check(name, scan, labels, voxel, connectivity, min_points=1, ignore=()):
    want = _want(name, scan, labels, voxel, connectivity, min_points, ignore)
    got = SO.extract_objects(scan, labels, voxel=voxel, connectivity=connectivity, min_points=min_points, ignore=ignore)
    _same(got, want)
    return got, want


def _room_min_points():
    scan, labels, _, voxel = _case("room")
    return OC.room_min_points(_want("room", scan, labels, voxel, 6)["object_points"])[0]


# ---- 1. every case against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_every_case_equals_the_restatement(name, connectivity):
    scan, labels, _, voxel = _case(name)
    got, want = _check(name, scan, labels, voxel, connectivity)
    assert got.n_objects >= 2 or name in ("serpentine", "slab")
    if name == "gap":
        assert got.n_objects == OC.GAP_OBJECTS[connectivity]
    if name == "checker":
        assert got.n_objects == got.n_units == 625
    if name == "mixed":
        assert got.object_labels.tolist() == list(OC.MIXED_CLASSES) and got.object_units.tolist() == [24, 24]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_labels_of_either_width_and_min_points(connectivity):
    scan, labels, _, voxel = _case("gap")
    a, _ = _check("gap", scan, labels, voxel, connectivity, min_points=7)  # the pairs hold 6 points, the blobs 24
    assert a.n_objects == 2 and a.n_dropped_points == 12 and a.n_components == OC.GAP_OBJECTS[connectivity]
    b = SO.extract_objects(scan, labels.astype(np.int32), voxel=voxel, connectivity=connectivity, min_points=7)
    _same(b, _want("gap", scan, labels, voxel, connectivity, 7))
    c, _ = _check("gap", scan, labels, voxel, connectivity, min_points=25)
    assert c.n_objects == 0 and c.object_lo.shape == (0, 3) and (c.objects == -1).all() and c.n_dropped_points == len(scan)


# ---- 2. one class: the partition of build_segments ----------------------------------------------------------------------------
def _grow_scans():
    return {"wrap": (C.wrap_case()[0], C.VOX), "serpentine": (C.serpentine_case()[0], C.VOX),
            "random": (C.random_case(0)[0], 0.05), "invalid": (C.with_invalid(C.random_case(1)[0], 11), 0.05),
            "room": (_case("room")[0], OC.ROOM_VOXEL)}


@pytest.mark.parametrize("connectivity,min_points", [(6, 1), (26, 4)])
@pytest.mark.parametrize("name", ["wrap", "serpentine", "random", "invalid", "room"])
def test_with_one_class_the_objects_are_the_segments_of_build_segments(name, connectivity, min_points):
    scan, voxel = _cached("grow-scans", _grow_scans)[name]
    seg = G.build_segments(scan, voxel, None, connectivity, min_points)
    got = SO.extract_objects(scan, np.full(len(scan), 3, np.int32), voxel, connectivity, min_points)
    assert torch.equal(got.objects, seg.segments) and torch.equal(got.object_points, seg.segment_points)
    assert torch.equal(got.unit_index, seg.voxel_index) and got.grid == seg.grid
    assert (got.n_objects, got.n_components, got.n_dropped_points, got.n_units, got.n_invalid) == (
        seg.n_segments, seg.n_components, seg.n_dropped_points, seg.n_voxels, seg.n_invalid)
    assert got.n_labels == 4 and (got.object_labels == 3).all() and got.n_unlabelled == 0


# ---- 3. the room ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_room_has_a_floor_walls_and_three_boxes(connectivity):
    scan, labels, _, voxel = _case("room")
    got, _ = _check("room", scan, labels, voxel, connectivity, min_points=_room_min_points())
    assert got.n_objects == 5 and got.object_labels.tolist() == [0, 1, 2, 2, 2]


def test_ignoring_the_floor_changes_no_other_object():
    scan, labels, _, voxel = _case("room")
    mp = _room_min_points()
    full, _ = _check("room", scan, labels, voxel, 26, mp)
    cut, _ = _check("room", scan, labels, voxel, 26, mp, ignore=(0,))
    assert cut.object_labels.tolist() == [1, 2, 2, 2] and cut.n_unlabelled == int((labels == 0).sum()) and cut.grid == full.grid
    obj_full, obj_cut = full.objects.cpu().numpy(), cut.objects.cpu().numpy()
    assert (obj_cut[labels == 0] == -1).all() and np.array_equal(obj_cut[labels != 0], obj_full[labels != 0] - 1 * (obj_full[labels != 0] >= 0))
    for name in ("object_points", "object_units", "object_lo", "object_hi", "object_centroid"):
        assert torch.equal(getattr(cut, name).view(torch.int32), getattr(full, name)[1:].view(torch.int32)), name


# ---- 4. points that take no part ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_negative_labels_and_non_finite_rows(connectivity):
    scan, labels, _, voxel = _case("room")
    bad_scan, bad_labels = _cached("bad-room", lambda: OC.with_bad_rows(scan, labels, 31))
    finite = np.isfinite(bad_scan[:, :3]).all(1)
    got, _ = _check("bad-room", bad_scan, bad_labels, voxel, connectivity, min_points=3)
    assert got.n_invalid == int((~finite).sum()) > 100 and got.n_unlabelled == int((finite & (bad_labels < 0)).sum()) > 100
    out = ~finite | (bad_labels < 0)
    assert (got.objects.cpu().numpy()[out] == -1).all() and (got.unit_index.cpu().numpy()[out] == -1).all()


def test_a_scan_without_a_participating_point():
    scan, labels, _, voxel = _case("slab")
    for name, s, l, ignore in (("none-negative", scan, np.full(len(scan), -1, np.int64), ()),
                               ("none-ignored", scan, labels, (2, 7)),
                               ("none-finite", np.full((50, 3), np.nan, f32), np.zeros(50, np.int64), ())):
        got, _ = _check(name, s, l, voxel, 26, ignore=ignore)
        assert got.n_objects == got.n_units == got.n_labels == 0 and (got.objects == -1).all() and (got.unit_index == -1).all()
        assert got.object_labels.numel() == 0 and got.object_centroid.shape == (0, 3)
    assert got.n_invalid == 50 and got.grid == (0, 0, 0)


def test_the_key_range_is_checked_before_the_sort(monkeypatch):
    """A label of 2^22 on a grid of 9 x 9 x 9 cells: 3 057 647 616 keys.  The ValueError names both numbers and comes after
    the first host read; nothing behind the bounds is launched."""
    launched = []
    for name in ("scene_obj_sort", "scene_obj_union", "scene_obj_components", "scene_obj_stats", "scene_obj_ids"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: launched.append(_n))
    scan = C.scan_of(np.array([[x, x, x] for x in range(9)]))
    labels = np.array([1] * 8 + [2 ** 22], np.int64)  # eight cells of class 1 along a diagonal, one point of a far class
    with pytest.raises(ValueError, match=r"%d labels .* 729 cells .*larger voxel or renumber" % (2 ** 22 + 1)):
        SO.extract_objects(scan, labels, voxel=C.VOX)
    with pytest.raises(ValueError, match="label above 2147483646"):
        SO.extract_objects(scan, np.where(labels > 1, 2 ** 40, labels), voxel=C.VOX)
    assert launched == []
    monkeypatch.undo()
    got = SO.extract_objects(scan, np.where(labels > 1, 2 ** 40, labels), voxel=C.VOX, ignore=(2 ** 40,))  # ignored: no key needed
    assert got.n_labels == 2 and got.n_unlabelled == 1 and got.n_objects == 1 and got.objects.tolist() == [0] * 8 + [-1]


# ---- 5. promises ------------------------------------------------------------------------------------------------------------------
def _fields(got):
    return ([getattr(got, k).cpu().numpy() for k, _ in INT_FIELDS] + [[getattr(got, k) for k in COUNTS]] +
            [getattr(got, k).cpu().numpy().view(np.uint32) for k in FLOAT_FIELDS])


def test_two_calls_and_a_host_scan_give_the_same_bits():
    scan, labels, _, voxel = _case("room")
    bad_scan, bad_labels = _cached("bad-room", lambda: OC.with_bad_rows(scan, labels, 31))
    dev, dev_labels = torch.from_numpy(bad_scan).cuda(), torch.from_numpy(bad_labels).cuda()
    a = SO.extract_objects(dev, dev_labels, voxel, 26, 3)
    b = SO.extract_objects(dev, dev_labels, voxel, 26, 3)
    c = SO.extract_objects(bad_scan, bad_labels, voxel, 26, 3)  # from the host
    d = SO.extract_objects(np.ascontiguousarray(bad_scan[:, :3]), dev_labels, voxel, 26, 3)  # three columns, labels on the device
    assert a.n_objects >= 5 and a.n_invalid > 100 and a.n_unlabelled > 100
    for other in (b, c, d):
        assert all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(other)))


# ---- 6. composition -----------------------------------------------------------------------------------------------------------------
def test_pool_segments_takes_the_objects_as_they_are():
    """A SceneResult of two classes built by hand, its labels turned into objects, the objects pooled: one mean logit row per
    object, by the pooling path that exists."""
    scan, _, _, voxel = _case("room")
    M = len(scan)
    rs = np.random.RandomState(41)
    votes = rs.randint(0, 3, M).astype(np.int32)
    scores = (rs.randn(M, 2) * 3).astype(f32) * np.maximum(votes, 1)[:, None].astype(f32)
    labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)
    res = scene.SceneResult(torch.from_numpy(labels).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(votes).cuda(), 1, 1,
                            int((labels == -1).sum()), 0)
    learner = fitted.FittedLearner.__new__(fitted.FittedLearner)  # the forwards need no model
    objs = learner.extract_objects(scan, res.labels, voxel=voxel, connectivity=26, min_points=4)
    want = _want("room-by-hand", scan, labels, voxel, 26, 4)
    _same(objs, want)
    assert objs.n_objects >= 2 and objs.n_unlabelled == int((labels < 0).sum()) > 0 and set(objs.object_labels.tolist()) == {0, 1}
    seg = SS.pool_segments(res, objs.objects)
    assert seg.n_segments == objs.n_objects and torch.equal(seg.segment_points, objs.object_points)
    ref = scene_segments_ref.pool(scores, votes, labels, want["objects"])
    assert np.array_equal(seg.labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(seg.segment_scores.cpu().numpy().view(np.uint32), ref["segment_scores"].view(np.uint32))
