"""Object instances from a labelled scan: which chairs, how many, and where.

predict_scene, predict_scene_sets and pool_segments end with one class per point; build_segments and grow_segments cut the
scan by geometry alone (without normal_tol a floor joins all that stands on it, with it a box falls into its faces).
extract_objects joins the two: points fall into the cells of build_segments' grid, the participating points of one class in
one cell are a UNIT, units of the same class in neighbouring cells are joined, and the connected components are the
objects -- each with its class, its points, its occupied cells, its axis-aligned box and its centroid.  Two classes that
share a cell are two units and never join, so every point of an object has the object's class.  The behaviour is defined
here ("Objects from a labelled scan", O1-O8; tests/scene_objects_ref.py restates it in numpy), since the
reference has no such function.  Like the rest of the scene path it draws no random number and sends no float through an
atomic: the union-find runs on integer atomics, the box on the order-preserving integer image of the float bits, the
centroid on 64-bit integer sums -- the same scan and labels give the same bits.

  1. finite points, their xyz extent; the largest participating label, the points
     left out by their label, labels that fit no key                                 r3d_scene_obj_bounds      host read 1 of 4
  2. keys label * n_cells + cell, stable sort of (key, scan index), unit heads and
     their scan, the unit table in ascending key order, the unit of every point      r3d_scene_obj_sort        host read 2 of 4
  3. every unit united with the units of its class in the cells in front of it       r3d_scene_obj_union
  4. roots, points per root, the roots with at least min_points points               r3d_scene_obj_components  host read 3 of 4
  5. per object its class, points, cells, box and centroid                           r3d_scene_obj_stats
  6. kept components numbered by ascending root, spread to the points                r3d_scene_obj_ids         host read 4 of 4

`objects` is a partition in the sense of pool_segments: pool_segments(res, objs.objects) gives the mean logits per object as
it stands.  It is also an int32 column a caller can append to a block's rows where a loader wants instance ids.

This module holds the host logic; the kernels are in csrc/scene_objects.hip, on the sort and the bounds of
csrc/scene_sort.hip and the union-find and component launches that csrc/scene_grow.hip shares (csrc/scene_components.h)."""
import numpy as np
import torch

from . import ops, scene
# read_record is looked up in this module at every call: tools/scene_objects_cost.py times the reads by replacing it here
from .scene_grow import _check_scan, _check_voxel, _on_device, _raise_on_error, extent_of, grid_of, read_record

MAX_IGNORE = ops.SCENE_OBJ_IGNORE
MAX_KEY = ops.SCENE_OBJ_KEY


class SceneObjects:
    """What extract_objects returns.  On the device: objects (M,) int32, 0 .. S - 1, or -1 for a point that takes no part or
    a point of a dropped component; object_labels (S,) int64, ascending; object_points (S,) int32; object_units (S,) int32,
    the occupied cells of the object; object_lo, object_hi (S, 3) fp32, the exact minima and maxima of its points; object_centroid
    (S, 3) fp32 (O8: within voxel / 512 plus rounding of the mean of its points); unit_index (M,) int32, the row of the
    point's unit in the unit table (ascending class, then cell key), -1 for a point that takes no part.  Host ints:
    n_objects (S), n_units, n_components (before min_points), n_dropped_points, n_unlabelled (finite points left out by their
    label), n_invalid (points with a non-finite coordinate), n_labels (the largest participating label plus one); grid
    (nx, ny, nz), (0, 0, 0) without a finite point."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def check_object_args(scan, labels, voxel=0.05, connectivity=26, min_points=1, ignore=()):
    """Raises ValueError before anything needs a device.  -> (scan, labels as tensors, voxel as float32, ignore as a sorted
    tuple of distinct ints)."""
    scan = _check_scan("extract_objects", scan, 3)
    if isinstance(labels, np.ndarray):
        labels = torch.from_numpy(labels)
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1:
        raise ValueError("extract_objects: labels must be (M,) integers, got %s" % (
            tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels).__name__,))
    if labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("extract_objects: labels must be int32 or int64, got %s" % labels.dtype)
    if labels.shape[0] != scan.shape[0]:
        raise ValueError("extract_objects: %d labels for %d points" % (labels.shape[0], scan.shape[0]))
    v32 = _check_voxel("extract_objects", voxel, connectivity, min_points)
    if not isinstance(ignore, (list, tuple, np.ndarray)) or not all(scene._is_int(c) and 0 <= int(c) < 2 ** 63 for c in ignore):
        raise ValueError("extract_objects: ignore %r must be a sequence of integer class ids >= 0" % (ignore,))
    ignore = tuple(sorted(set(int(c) for c in ignore)))
    if len(ignore) > MAX_IGNORE:
        raise ValueError("extract_objects: %d ignored classes (at most %d)" % (len(ignore), MAX_IGNORE))
    return scan, labels, v32, ignore


def check_key_range(n_labels, grid):
    """O3: a key is label * n_cells + cell and the points that take no part get n_labels * n_cells, which must fit an int32.
    -> n_labels * n_cells; raises ValueError, naming both numbers, when that exceeds 2^31 - 1."""
    n_cells = int(grid[0]) * int(grid[1]) * int(grid[2])
    if int(n_labels) * n_cells > MAX_KEY:
        raise ValueError("extract_objects: %d labels (the largest participating label plus one) times %d cells (%d x %d x %d) "
                         "exceed 2^31 - 1 keys; use a larger voxel or renumber the classes" % (
                             int(n_labels), n_cells, grid[0], grid[1], grid[2]))
    return int(n_labels) * n_cells


def _empty(M, dev, n_invalid, n_unlabelled, grid):
    none = torch.full((M,), -1, device=dev, dtype=torch.int32)
    table = lambda dtype, *shape: torch.empty(0, *shape, device=dev, dtype=dtype)
    return SceneObjects(objects=none, unit_index=none.clone(), object_labels=table(torch.int64),
                        object_points=table(torch.int32), object_units=table(torch.int32), object_lo=table(torch.float32, 3),
                        object_hi=table(torch.float32, 3), object_centroid=table(torch.float32, 3), n_objects=0, n_units=0,
                        n_components=0, n_dropped_points=0, n_unlabelled=n_unlabelled, n_invalid=n_invalid, n_labels=0, grid=grid)


def extract_objects(scan, labels, voxel=0.05, connectivity=26, min_points=1, ignore=()):
    """scan (M, >= 3) float32 rows x y z ..., host or device, M <= 2^27 (only x y z are read); labels (M,) int32 or int64, host
    or device: the labels of a SceneResult, SceneSetsResult or SegmentResult, or ground truth; a negative label means "no
    class" -> SceneObjects.  ignore: class ids that form no objects, e.g. (0,) for a background; voxel: the edge of a cell, at
    most 1024 of them along an axis; connectivity 6 (faces) or 26 (faces, edges, corners); min_points: an object with fewer
    points is dropped, its points get -1.  The result's .objects goes to pool_segments as it is: pool_segments(res,
    objs.objects) gives the mean logits per object.  There is no CPU path.  See the module text and INTEGRATION.md, "Objects
    from a labelled scan"."""
    scan, labels, voxel, ignore = check_object_args(scan, labels, voxel, connectivity, min_points, ignore)
    dev, scan = _on_device("extract_objects", scan, 3, labels)
    labels = labels.to(dev).contiguous()
    ignored = torch.tensor(ignore, device=dev, dtype=torch.int64) if ignore else None
    M = scan.shape[0]
    ws = ops.scene_obj_workspace(M, dev)
    ops.scene_obj_bounds(scan, labels, ignored, ws)
    rec = read_record(ws)  # host read 1 of 4
    n_valid, n_points, n_labels = rec[ops.GROW_R_NVALID], rec[ops.OBJ_R_NPOINTS], rec[ops.OBJ_R_NLABELS]
    n_unlabelled = rec[ops.OBJ_R_NUNLABELLED]
    if rec[ops.OBJ_R_NOVER]:
        raise ValueError("extract_objects: %d points have a label above %d, which no key holds; renumber the classes"
                         % (rec[ops.OBJ_R_NOVER], ops.SCENE_OBJ_LABEL))
    if n_valid == 0:
        return _empty(M, dev, M, 0, (0, 0, 0))
    lo, hi = extent_of(rec)
    grid = grid_of(lo, hi, voxel)
    if n_points == 0:  # O1: no point takes part, nothing else is launched
        return _empty(M, dev, M - n_valid, n_unlabelled, grid)
    check_key_range(n_labels, grid)
    unit_index = ops.scene_obj_sort(scan, labels, ignored, lo, voxel, grid, n_labels, n_points, ws)
    U = read_record(ws)[ops.GROW_R_V]  # host read 2 of 4
    ops.scene_obj_union(M, grid, n_labels, U, connectivity, ws)
    ops.scene_obj_components(M, U, min_points, ws)
    rec = read_record(ws)  # host read 3 of 4: the tables' sizes
    _raise_on_error("extract_objects", rec)
    n_components, S = rec[ops.GROW_R_NCOMP], rec[ops.GROW_R_S]
    if S:
        o_labels, o_points, o_units, o_lo, o_hi, o_centroid = ops.scene_obj_stats(scan, lo, voxel, grid, n_labels, U, S, ws)
    else:
        e = _empty(M, dev, 0, 0, grid)
        o_labels, o_points, o_units = e.object_labels, e.object_points, e.object_units
        o_lo, o_hi, o_centroid = e.object_lo, e.object_hi, e.object_centroid
    objects = ops.scene_obj_ids(unit_index, U, S, ws)
    rec = read_record(ws)  # host read 4 of 4, after everything is queued
    _raise_on_error("extract_objects", rec)
    return SceneObjects(objects=objects, unit_index=unit_index, object_labels=o_labels, object_points=o_points,
                        object_units=o_units, object_lo=o_lo, object_hi=o_hi, object_centroid=o_centroid, n_objects=S, n_units=U,
                        n_components=n_components, n_dropped_points=rec[ops.GROW_R_NDROPPED], n_unlabelled=n_unlabelled,
                        n_invalid=M - n_valid, n_labels=n_labels, grid=grid)
