"""absorb_segments, that is grow_segments with absorb ("Building segments", G6a) restated in numpy on top of tests/scene_grow_ref.py
and tests/scene_grow_normals_ref.py: the GPU tests compare the kernels with it bit for bit.  Everything is integer.

  A1  owner_0[v] = root[v] (G5) when the component of v is kept by G6, else -1: v is FREE; ring[v] = 0, or -1 when free;
  A2  round r = 1 .. R, for every v free in owner_{r-1}: its neighbours are the occupied voxels at all 6 or 26 offsets,
      found by their coordinates; N = those with owner_{r-1} >= 0; N empty: v stays free; else owner_r[v] = the owner that
      most of N have, the smallest on a tie, and ring[v] = r.  A round reads owner_{r-1} only (two tables);
  A3  a voxel with owner_R[v] = t >= 0 belongs to the component of root t; the kept components are numbered as without
      absorb (G7); segment_points counts the absorbed points, n_dropped_points the points of the voxels still free.

A neighbour is looked up by its coordinate triple in a dictionary of the occupied voxels, as in scene_grow_ref.grow."""
import collections

import numpy as np

import scene_grow_normals_ref as N
import scene_grow_ref as R

MAX_RINGS = 64


def absorb(out, connectivity, rings):
    """out: the dict of scene_grow_ref.grow or scene_grow_normals_ref.grow (left as it is) -> a new dict with the same fields
    after `rings` rounds, and voxel_ring (V,) int32 (None with rings = 0), n_absorbed_voxels, n_absorbed_points."""
    assert isinstance(rings, int) and 0 <= rings <= MAX_RINGS
    res = dict(out, voxel_ring=None, n_absorbed_voxels=0, n_absorbed_points=0)
    if rings == 0:
        return res
    V = out["n_voxels"]
    if V == 0:
        res["voxel_ring"] = np.zeros(0, np.int32)
        return res
    nx, ny, nz = out["grid"]
    keys, vpoints, root = out["voxel_keys"], out["voxel_points"].astype(np.int64), out["voxel_component"]
    vcoord = np.stack([keys % nx, (keys // nx) % ny, keys // (nx * ny)], 1).tolist()
    row_of = {tuple(c): v for v, c in enumerate(vcoord)}
    valid = out["voxel_index"] >= 0
    row = out["voxel_index"][valid]
    seg_of_voxel = np.full(V, -1, np.int64)
    seg_of_voxel[row] = out["segments"][valid]  # the points of a voxel share their segment
    owner = np.where(seg_of_voxel >= 0, root, -1).astype(np.int64)  # A1
    ring = np.where(owner >= 0, 0, -1).astype(np.int32)
    offs = R.offsets(connectivity)
    neighbours = {}
    for v in np.flatnonzero(owner < 0).tolist():
        ix, iy, iz = vcoord[v]
        neighbours[v] = [b for b in (row_of.get((ix + dx, iy + dy, iz + dz)) for dx, dy, dz in offs) if b is not None]
    for r in range(1, rings + 1):  # A2
        new = owner.copy()
        for v, nb in neighbours.items():
            if owner[v] >= 0:
                continue
            tally = collections.Counter(int(owner[b]) for b in nb if owner[b] >= 0)
            if tally:
                new[v] = min(tally, key=lambda t: (-tally[t], t))
                ring[v] = r
        owner = new
    kept_roots = np.unique(owner[ring == 0])  # A3: ascending roots, the ids of G7
    assert len(kept_roots) == out["n_segments"] and np.array_equal(seg_of_voxel[kept_roots], np.arange(len(kept_roots)))
    new_seg = np.where(owner >= 0, np.searchsorted(kept_roots, np.maximum(owner, 0)), -1).astype(np.int32)
    segments = np.full(len(out["segments"]), -1, np.int32)
    segments[valid] = new_seg[row]
    taken = ring > 0
    sizes = np.bincount(new_seg[owner >= 0], weights=vpoints[owner >= 0], minlength=len(kept_roots))
    res.update(segments=segments, segment_points=sizes.astype(np.int32), n_dropped_points=int(vpoints[owner < 0].sum()),
               voxel_ring=ring, n_absorbed_voxels=int(taken.sum()), n_absorbed_points=int(vpoints[taken].sum()),
               voxel_owner=owner)
    return res


def grow(scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None, absorb_rings=0):
    """scene_grow_normals_ref.grow (which is scene_grow_ref.grow without normal_tol), then absorb."""
    return absorb(N.grow(scan, voxel, colour_tol, connectivity, min_points, normal_tol=normal_tol), connectivity, absorb_rings)
