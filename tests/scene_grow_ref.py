"""build_segments ("Building segments", G1-G7) restated in numpy: the GPU tests compare the kernels with it
bit for bit.

  G1  a point is valid when x, y, z are finite; any other point gets segments = voxel_index = -1;
  G2  v0 = the per-axis minimum of the valid points; i_a = floor((v_a - v0_a) / voxel) in float32, one subtraction and one
      division; n_a = that at the axis maximum, plus 1; key = (iz * ny + iy) * nx + ix;
  G3  the occupied voxels in ascending key order; a voxel's points in ascending scan index; its mean colour: the rows'
      columns 3 .. 5 summed by scene_segments_ref.pool_rows (tiles of 256, one addition at a time), divided by float32(count);
  G4  voxels a != b are joined when both are occupied, their COORDINATES differ by at most 1 on every axis (connectivity 6:
      on exactly one axis) and, with colour_tol, |mean_c(a) - mean_c(b)| <= colour_tol for every channel in float32;
  G5  the connected components; the root of one is its smallest voxel row;
  G6  a component with fewer than min_points points is dropped, its points get -1;
  G7  the kept components are numbered 0 .. S - 1 by ascending root.

A neighbour is looked up by its coordinate triple in a dictionary of the occupied voxels: no key arithmetic finds one."""
import numpy as np

import scene_segments_ref

f32 = np.float32
MAX_AXIS = 1024


def offsets(connectivity):
    """The (dx, dy, dz) of a neighbourhood: 6 or 26 of them."""
    assert connectivity in (6, 26)
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = abs(dx) + abs(dy) + abs(dz)
                if n == 1 or (connectivity == 26 and n > 1):
                    out.append((dx, dy, dz))
    return out


def voxels_of(scan, voxel):
    """scan (M, >= 3) float32 -> (valid (M,) bool, v0 (3,) float32, coords (n_valid, 3) int64 as ix iy iz, grid (nx, ny, nz)) by
    G1 and G2; v0 None and grid (0, 0, 0) without a valid point."""
    scan = np.asarray(scan)
    assert scan.dtype == f32 and scan.ndim == 2
    xyz = scan[:, :3]
    valid = np.isfinite(xyz).all(1)
    if not valid.any():
        return valid, None, np.zeros((0, 3), np.int64), (0, 0, 0)
    pts = xyz[valid]
    v0, v1 = pts.min(0), pts.max(0)
    s = f32(voxel)
    cell = lambda v: np.floor((v - v0) / s)  # float32 - float32, float32 / float32: every operation rounded on its own
    q = cell(pts)
    assert q.dtype == f32
    grid = tuple(int(n) + 1 for n in cell(v1))
    return valid, v0, q.astype(np.int64), grid


def grow(scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1):
    """-> a dict with the fields of scene_grow.GrownSegments as numpy arrays and ints, and the voxel table: voxel_keys (V,)
    int64, voxel_points (V,) int32, voxel_means (V, 3) float32 (with colour_tol), voxel_component (V,) the root of every row."""
    scan = np.asarray(scan)
    M = scan.shape[0]
    valid, v0, coords, (nx, ny, nz) = voxels_of(scan, voxel)
    assert max(nx, ny, nz) <= MAX_AXIS
    segments, voxel_index = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    out = dict(segments=segments, voxel_index=voxel_index, segment_points=np.zeros(0, np.int32), n_segments=0, n_voxels=0,
               n_components=0, n_dropped_points=0, n_invalid=int(M - valid.sum()), grid=(nx, ny, nz))
    if not valid.any():
        return out
    keys = (coords[:, 2] * ny + coords[:, 1]) * nx + coords[:, 0]
    vkeys, inverse = np.unique(keys, return_inverse=True)  # ascending keys
    V = len(vkeys)
    scan_index = np.flatnonzero(valid)  # ascending: a voxel's points come out in scan order below
    voxel_index[scan_index] = inverse.astype(np.int32)
    members = [[] for _ in range(V)]
    for p, v in zip(scan_index.tolist(), inverse.tolist()):
        members[v].append(p)
    vpoints = np.array([len(m) for m in members], np.int32)
    vcoord = np.stack([vkeys % nx, (vkeys // nx) % ny, vkeys // (nx * ny)], 1)
    row_of = {tuple(c): v for v, c in enumerate(vcoord.tolist())}
    means = None
    if colour_tol is not None:
        means = np.zeros((V, 3), f32)
        with np.errstate(invalid="ignore", over="ignore"):
            for v, m in enumerate(members):
                means[v] = scene_segments_ref.pool_rows(np.ascontiguousarray(scan[m, 3:6])) / f32(len(m))
    parent = list(range(V))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    offs = offsets(connectivity)
    tol = None if colour_tol is None else f32(colour_tol)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, (ix, iy, iz) in enumerate(vcoord.tolist()):
            for dx, dy, dz in offs:
                b = row_of.get((ix + dx, iy + dy, iz + dz))
                if b is None:
                    continue
                if tol is not None and not bool((np.abs(means[a] - means[b]) <= tol).all()):  # a NaN joins nothing
                    continue
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)  # the root of a component: its smallest row
    root = np.array([find(v) for v in range(V)], np.int64)
    cnt = np.zeros(V, np.int64)
    np.add.at(cnt, root, vpoints)
    is_root = root == np.arange(V)
    kept = is_root & (cnt >= min_points)
    seg_of_root = np.full(V, -1, np.int32)
    seg_of_root[kept] = np.arange(int(kept.sum()), dtype=np.int32)
    segments[scan_index] = seg_of_root[root[inverse]]
    out.update(segment_points=cnt[kept].astype(np.int32), n_segments=int(kept.sum()), n_voxels=V, n_components=int(is_root.sum()),
               n_dropped_points=int(cnt[is_root & ~kept].sum()), voxel_keys=vkeys, voxel_points=vpoints, voxel_means=means,
               voxel_component=root)
    return out
