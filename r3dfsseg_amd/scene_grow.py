"""Segments grown from the scan itself: the partition that scene_segments.pool_segments takes, built on the device.

pool_segments needs a partition of the scan's points, and the reference only ever reads one that an offline script wrote
(dataloaders/loader.py:339-349).  build_segments makes one from a raw `x y z [r g b]` scan by the simplest useful criterion,
adjacency, colour and surface normal: points fall into voxels, occupied voxels that touch -- and, with colour_tol, whose
mean colours agree, and, with normal_tol, whose normals agree -- are joined, the connected components are the segments.
Adjacency alone joins a floor to every wall and to what stands on it; normal_tol is plane-wise region growing: a voxel's
normal comes from the centroids of the occupied voxels among the 27 around it, by a fixed sequence of fp32 operations (no
eigen-solver), and two neighbours are joined only when the angle between their normals is at most normal_tol degrees.  The
behaviour is defined here ("Building segments", G1-G7 with G3c and G3n; tests/scene_grow_ref.py and
tests/scene_grow_normals_ref.py restate it in numpy).  Like the rest of the scene path it draws no random number and adds
no float by an atomic; the union-find runs on integer atomics, and the component a voxel ends in depends on the graph
alone, so the same scan gives the same bits.

  1. valid points, their xyz extent                                               r3d_scene_grow_bounds      host read 1 of 4
  2. voxel keys, stable sort of (key, scan index), voxel heads and their scan     r3d_scene_grow_sort        host read 2 of 4
  3. the voxel table in ascending key order, the voxel of every point, mean
     colours in the summation order of pool_segments                              r3d_scene_grow_voxels
  3c. with normal_tol: the centroid of every voxel, inside the voxel             r3d_scene_grow_centroids
  3n. with normal_tol: the normal and the support of every voxel                  r3d_scene_grow_normals
  4. every voxel united with the occupied neighbours in front of it               r3d_scene_grow_union, or with normal_tol
                                                                                  r3d_scene_grow_union_normals
  5. roots, points per root, the roots with at least min_points points            r3d_scene_grow_components  host read 3 of 4
  5a. absorb_segments with absorb > 0: the voxels of dropped components taken, ring by ring, into
      the kept component most of their neighbours belong to (G6a)                 r3d_scene_grow_absorb
  6. kept components numbered by ascending root, spread to the points             r3d_scene_grow_ids         host read 4 of 4

This module holds the host logic; the kernels are in csrc/scene_grow.hip, on the sort and the bounds of csrc/scene_sort.hip."""
import math

import numpy as np
import torch

from . import ops, scene

MAX_AXIS = ops.SCENE_GROW_AXIS
MAX_RINGS = ops.SCENE_GROW_RINGS
AXES = "xyz"


class GrownSegments:
    """What build_segments, grow_segments and absorb_segments return.  On the device: segments (M,) int32, 0 .. S - 1, or -1 for an invalid point or a point
    of a dropped component; segment_points (S,) int32; voxel_index (M,) int32, the row of the point's voxel in the voxel
    table (ascending key order), -1 for an invalid point; voxel_means (V, 3) fp32, the mean colour of every voxel, None
    without colour_tol.  With normal_tol, else None: voxel_centroids (V, 3) fp32, the mean position of a voxel's points
    measured from the voxel's lower corner; voxel_normals (V, 3) fp32, not of unit length, its largest component 1, a row of
    NaNs where a voxel has no normal; voxel_support (V,) int32, the occupied voxels among the 27 around it.  With absorb > 0,
    else None: voxel_ring (V,) int32, 0 for a voxel of a kept component, r for one absorbed in round r, -1 for one still
    free.  Host ints: n_segments (S), n_voxels, n_components (before min_points), n_dropped_points (after absorbing),
    n_absorbed_voxels, n_absorbed_points (0 with absorb=0), n_invalid; grid (nx, ny, nz), (0, 0, 0) without a valid point."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _is_real(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def cos2_of(normal_tol):
    """The threshold of the normal test (G4): float32(cos(radians(normal_tol)) ** 2), computed in float64, rounded once."""
    return np.float32(math.cos(math.radians(float(normal_tol))) ** 2)


def _check_scan(what, scan, min_columns):
    """The scan of `what` (the function named in the messages): (M, 3) or (M, >= min_columns) float32, M <= 2^27 -> a tensor."""
    if isinstance(scan, np.ndarray):
        scan = torch.from_numpy(scan)
    is_tensor = isinstance(scan, torch.Tensor)
    if not is_tensor or scan.dim() != 2 or scan.shape[0] < 1 or not (scan.shape[1] == 3 or scan.shape[1] >= min_columns):
        rows = "(M, >= 3) rows `x y z ...`" if min_columns == 3 else "(M, 3) rows `x y z` or (M, >= 6) rows `x y z r g b ...`"
        raise ValueError("%s: scan must be %s, got %s" % (what, rows, tuple(scan.shape) if is_tensor else type(scan).__name__))
    if scan.dtype != torch.float32:
        raise ValueError("%s: scan must be float32, got %s" % (what, scan.dtype))
    if scan.shape[0] > scene.MAX_POINTS:
        raise ValueError("%s: %d points (at most 2^27)" % (what, scan.shape[0]))
    return scan


def _check_voxel(what, voxel, connectivity, min_points):
    """-> voxel as float32."""
    with np.errstate(over="ignore", under="ignore"):
        v32 = np.float32(voxel) if _is_real(voxel) else np.float32(np.nan)
    if not (_is_real(voxel) and np.isfinite(voxel) and voxel > 0 and np.isfinite(v32) and v32 > 0):
        raise ValueError("%s: voxel %r must be a finite float > 0 (in float32 too)" % (what, voxel))
    if not scene._is_int(connectivity) or int(connectivity) not in (6, 26):
        raise ValueError("%s: connectivity %r must be 6 or 26" % (what, connectivity))
    if not scene._is_int(min_points) or min_points < 1:
        raise ValueError("%s: min_points %r must be an integer >= 1" % (what, min_points))
    return v32


def _check_colour(what, colour_tol, scan):
    """colour_tol: None, or finite and >= 0 (in float32 too), and then the scan has colour columns."""
    if colour_tol is None:
        return
    with np.errstate(over="ignore", under="ignore"):
        t32 = np.float32(colour_tol) if _is_real(colour_tol) else np.float32(np.nan)
    if not (_is_real(colour_tol) and np.isfinite(colour_tol) and colour_tol >= 0 and np.isfinite(t32)):
        raise ValueError("%s: colour_tol %r must be None or a finite float >= 0" % (what, colour_tol))
    if scan.shape[1] < 6:
        raise ValueError("%s: colour_tol %r given, but a scan of %d columns has no colour (x y z r g b)"
                         % (what, colour_tol, scan.shape[1]))


def check_grow_args(scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None, absorb=0):
    """Raises ValueError before anything needs a device.  -> (scan as a tensor, voxel as float32)."""
    scan = _check_scan("build_segments", scan, 6)
    v32 = _check_voxel("build_segments", voxel, connectivity, min_points)
    _check_colour("build_segments", colour_tol, scan)
    if normal_tol is not None and not (_is_real(normal_tol) and np.isfinite(normal_tol) and 0 <= normal_tol <= 90):
        raise ValueError("grow_segments: normal_tol %r must be None or a finite real number of degrees in [0, 90]" % (normal_tol,))
    if not scene._is_int(absorb) or not 0 <= absorb <= MAX_RINGS:
        raise ValueError("absorb_segments: absorb %r must be an integer number of rings in 0 .. %d" % (absorb, MAX_RINGS))
    return scan, v32


def grid_of(lo, hi, voxel, what="build_segments"):
    """lo, hi (3,) float32 minima and maxima of the valid points -> (nx, ny, nz) by G2: the keys kernel's arithmetic at the
    maximum, plus one.  Raises ValueError in the name of `what`, naming the axis, when one of them exceeds MAX_AXIS."""
    grid = tuple(scene.n_cells_along(lo[a], hi[a], voxel) for a in range(3))
    for a, n in enumerate(grid):
        if n > MAX_AXIS:
            extent = float(np.float32(hi[a]) - np.float32(lo[a]))
            raise ValueError("%s: %d voxels of %g along %s (at most %d per axis); the extent %g fits with any voxel "
                             "above %.9g" % (what, n, float(voxel), AXES[a], MAX_AXIS, extent, extent / MAX_AXIS))
    return grid


def read_record(ws):
    """The record in front of the workspace as host ints: a host read (the call has at most four)."""
    return ws[:ops.SCENE_GROW_REC].tolist()


def _raise_on_error(what, rec):
    if rec[ops.GROW_R_ERROR]:
        raise RuntimeError("%s: the union-find ran out of its bounded loops (error word %d: bit 0 a find, bit 1 a "
                           "unite): its table is corrupted, no result" % (what, rec[ops.GROW_R_ERROR]))


def extent_of(rec):
    """-> (lo, hi), (3,) float32 each: the minima and maxima of the valid points, from the float bits in the record."""
    ext = np.array(rec[ops.GROW_R_MIN:ops.GROW_R_MIN + 6], np.int32).view(np.float32)
    return ext[:3], ext[3:]


def _on_device(what, scan, columns, *others):
    """-> (the device of the first of scan and `others` that is on one, else the current one; the scan there, contiguous).
    The kernels take rows of up to 64 floats and only ever read the first `columns`.  There is no CPU path."""
    if not torch.cuda.is_available():
        raise RuntimeError("%s: no device (there is no CPU path)" % what)
    on = [t.device for t in (scan,) + others if t.is_cuda]
    dev = on[0] if on else torch.device("cuda", torch.cuda.current_device())
    return dev, (scan[:, :columns] if scan.shape[1] > 64 else scan).to(dev).contiguous()


def build_segments(scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1):
    """grow_segments without normal_tol: adjacency and, with colour_tol, colour.  Its signature is kept as it was; the
    normal criterion is a keyword of grow_segments."""
    return grow_segments(scan, voxel, colour_tol, connectivity, min_points)


def grow_segments(scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None):
    """absorb_segments without absorbing: build_segments and, with normal_tol, the normal test.  Its signature is kept as it
    was (a test pins it); the rings are a keyword of absorb_segments."""
    return absorb_segments(scan, voxel, colour_tol, connectivity, min_points, normal_tol)


def absorb_segments(scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None, absorb=0):
    """scan (M, 3) or (M, >= 6) float32 rows x y z [r g b ...], host or device, M <= 2^27 -> GrownSegments.  voxel: the edge
    of a voxel, at most 1024 of them along an axis; connectivity 6 (faces) or 26 (faces, edges, corners); colour_tol: None,
    or the largest difference of two neighbouring voxels' mean colours, per channel, that still joins them; min_points: a
    component with fewer points is dropped, its points get -1; normal_tol: None, or the largest angle in degrees, 0 .. 90,
    between the normals of two neighbouring voxels that still joins them (both must have a normal; with colour_tol both
    tests must hold; needs no colour); absorb: the number of rings, 0 .. 64, by which the voxels of dropped components are
    taken into the kept segment most of their neighbours belong to (G6a: no colour or normal test; S and every id of
    absorb=0 stay, only -1s become ids).  See the module text and INTEGRATION.md, "Building segments"."""
    scan, voxel = check_grow_args(scan, voxel, colour_tol, connectivity, min_points, normal_tol, absorb)
    absorb = int(absorb)
    dev, scan = _on_device("build_segments", scan, 6)
    M = scan.shape[0]
    ws = ops.scene_grow_workspace(M, dev)
    ops.scene_grow_bounds(scan, ws)
    rec = read_record(ws)  # host read 1 of 4
    n_valid = rec[ops.GROW_R_NVALID]
    if n_valid == 0:  # G1: nothing else is launched
        none = torch.full((M,), -1, device=dev, dtype=torch.int32)
        table = lambda on, *shape: torch.empty(0, *shape, device=dev, dtype=torch.float32) if on else None
        return GrownSegments(segments=none, segment_points=torch.empty(0, device=dev, dtype=torch.int32), voxel_index=none.clone(),
                             voxel_means=table(colour_tol is not None, 3), n_segments=0, n_voxels=0, n_components=0,
                             n_dropped_points=0, n_invalid=M, grid=(0, 0, 0), voxel_centroids=table(normal_tol is not None, 3),
                             voxel_normals=table(normal_tol is not None, 3),
                             voxel_support=None if normal_tol is None else torch.empty(0, device=dev, dtype=torch.int32),
                             voxel_ring=torch.empty(0, device=dev, dtype=torch.int32) if absorb else None,
                             n_absorbed_voxels=0, n_absorbed_points=0)
    lo, hi = extent_of(rec)
    grid = grid_of(lo, hi, voxel)
    ops.scene_grow_sort(scan, lo, voxel, grid, ws)
    V = read_record(ws)[ops.GROW_R_V]  # host read 2 of 4
    voxel_index, voxel_means = ops.scene_grow_voxels(scan, grid, n_valid, V, colour_tol is not None, ws)
    centroids = normals = support = None
    if normal_tol is None:
        ops.scene_grow_union(M, grid, V, connectivity, voxel_means, colour_tol, ws)
    else:
        centroids = ops.scene_grow_centroids(scan, lo, voxel, grid, V, ws)
        normals, support = ops.scene_grow_normals(M, grid, V, voxel, centroids, ws)
        ops.scene_grow_union_normals(M, grid, V, connectivity, voxel_means, colour_tol, normals, cos2_of(normal_tol), ws)
    ops.scene_grow_components(M, V, min_points, ws)
    rec = read_record(ws)  # host read 3 of 4: the tables' sizes
    _raise_on_error("build_segments", rec)
    n_components, S = rec[ops.GROW_R_NCOMP], rec[ops.GROW_R_S]
    ring = ops.scene_grow_absorb(M, grid, V, connectivity, absorb, ws) if absorb else None
    segments, segment_points = ops.scene_grow_ids(voxel_index, V, S, ws)
    rec = read_record(ws)  # host read 4 of 4, after everything is queued
    _raise_on_error("build_segments", rec)
    return GrownSegments(segments=segments, segment_points=segment_points, voxel_index=voxel_index, voxel_means=voxel_means,
                         n_segments=S, n_voxels=V, n_components=n_components, n_dropped_points=rec[ops.GROW_R_NDROPPED],
                         n_invalid=M - n_valid, grid=grid, voxel_centroids=centroids, voxel_normals=normals, voxel_support=support,
                         voxel_ring=ring, n_absorbed_voxels=rec[ops.GROW_R_ABSORBED_VOXELS],
                         n_absorbed_points=rec[ops.GROW_R_ABSORBED_POINTS])
