"""extract_objects ("Objects from a labelled scan", O1-O8) restated in numpy with plain loops and
dictionaries: the GPU tests compare the kernels with it bit for bit.

  O1  a point takes part when x, y, z are finite, its label is >= 0 and not in `ignore`; any other point gets objects =
      unit_index = -1; n_invalid counts the non-finite points, n_unlabelled the finite ones left out by their label;
  O2  the grid of build_segments (scene_grow_ref.voxels_of): its origin is the minimum over the FINITE points;
  O3  a unit: the participating points of one class in one cell; key = label * n_cells + cell; n_labels = the largest
      participating label + 1; n_labels * n_cells <= 2^31 - 1;
  O4  units a != b are neighbours when they have the same class and their cell COORDINATES differ by at most 1 on every axis
      (connectivity 6: on exactly one axis);
  O5  the connected components; the root of one is its smallest unit row;
  O6  a component with fewer than min_points points is dropped; the kept ones are numbered by ascending root;
  O7  per object and axis the minimum and maximum of its points' float32 coordinates, -0.0 below +0.0;
  O8  u = floor(((v - v0) / voxel) * 256) in float32, every operation rounded, clamped to 0 .. 256 n - 1; summed as integers;
      the centroid in float64: v0 + voxel * ((sum / n) + 0.5) / 256, rounded once to float32.

A neighbour is looked up by (class, coordinate triple) in a dictionary of the units: no key arithmetic finds one."""
import numpy as np

import scene_grow_ref as R

f32, f64 = np.float32, np.float64
MAX_KEY = 2 ** 31 - 1
SUB = 256


def image(x):
    """The order-preserving integer image of float32 values (O7): int32, its own inverse on the bits."""
    bits = np.asarray(x, f32).view(np.int32)
    return np.where(bits >= 0, bits, bits ^ np.int32(0x7fffffff))


def unimage(i):
    i = np.asarray(i, np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7fffffff)).astype(np.int32).view(f32)


def centroid_of(v0, voxel, total, n):
    """O8 in float64, the operations in the stated order, rounded once."""
    return f32(f64(v0) + f64(voxel) * ((f64(total) / f64(n)) + f64(0.5)) / f64(SUB))


def extract(scan, labels, voxel=0.05, connectivity=26, min_points=1, ignore=()):
    """-> a dict with the fields of scene_objects.SceneObjects as numpy arrays and ints, and the unit table: unit_keys (U,)
    int64, unit_points (U,) int32, unit_component (U,) the root of every row."""
    scan, labels = np.asarray(scan), np.asarray(labels)
    assert labels.dtype in (np.int32, np.int64) and labels.shape == (scan.shape[0],)
    M = scan.shape[0]
    valid, v0, coords, (nx, ny, nz) = R.voxels_of(scan, voxel)
    assert max(nx, ny, nz) <= R.MAX_AXIS
    lab = labels.astype(np.int64)
    part = valid & (lab >= 0)
    for c in ignore:
        part &= lab != int(c)
    objects, unit_index = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    out = dict(objects=objects, unit_index=unit_index, object_labels=np.zeros(0, np.int64), object_points=np.zeros(0, np.int32),
               object_units=np.zeros(0, np.int32), object_lo=np.zeros((0, 3), f32), object_hi=np.zeros((0, 3), f32),
               object_centroid=np.zeros((0, 3), f32), n_objects=0, n_units=0, n_components=0, n_dropped_points=0,
               n_unlabelled=int((valid & ~part).sum()), n_invalid=int(M - valid.sum()), n_labels=0, grid=(nx, ny, nz),
               unit_keys=np.zeros(0, np.int64), unit_points=np.zeros(0, np.int32), unit_component=np.zeros(0, np.int64))
    if not part.any():
        return out
    n_labels, n_cells = int(lab[part].max()) + 1, nx * ny * nz
    assert n_labels * n_cells <= MAX_KEY
    cell_of = {}  # scan index -> (ix, iy, iz)
    for p, c in zip(np.flatnonzero(valid).tolist(), coords.tolist()):
        cell_of[p] = tuple(c)
    members = {}  # (label, ix, iy, iz) -> scan indices, ascending
    for p in np.flatnonzero(part).tolist():
        members.setdefault((int(lab[p]),) + cell_of[p], []).append(p)
    key_of = lambda u: u[0] * n_cells + (u[3] * ny + u[2]) * nx + u[1]
    units = sorted(members, key=key_of)  # ascending key: ascending class, then cell key
    U = len(units)
    row_of = {u: r for r, u in enumerate(units)}
    for r, u in enumerate(units):
        unit_index[members[u]] = r
    upoints = np.array([len(members[u]) for u in units], np.int32)
    parent = list(range(U))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    offs = R.offsets(connectivity)
    for a, (l, ix, iy, iz) in enumerate(units):
        for dx, dy, dz in offs:
            b = row_of.get((l, ix + dx, iy + dy, iz + dz))
            if b is None:
                continue
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)  # the root of a component: its smallest row
    root = np.array([find(v) for v in range(U)], np.int64)
    cnt = np.zeros(U, np.int64)
    np.add.at(cnt, root, upoints)
    is_root = root == np.arange(U)
    kept = is_root & (cnt >= min_points)
    S = int(kept.sum())
    obj_of_root = np.full(U, -1, np.int32)
    obj_of_root[kept] = np.arange(S, dtype=np.int32)
    lo_i = np.full((S, 3), np.iinfo(np.int32).max, np.int32)
    hi_i = np.full((S, 3), np.iinfo(np.int32).min, np.int32)
    total = [[0, 0, 0] for _ in range(S)]
    n_units = np.zeros(S, np.int32)
    s32, top = f32(voxel), [SUB * nx - 1, SUB * ny - 1, SUB * nz - 1]
    for r, u in enumerate(units):
        s = int(obj_of_root[root[r]])
        objects[members[u]] = s
        if s < 0:
            continue
        n_units[s] += 1
        pts = scan[members[u], :3]
        im = image(pts)
        lo_i[s], hi_i[s] = np.minimum(lo_i[s], im.min(0)), np.maximum(hi_i[s], im.max(0))
        sub = np.floor(((pts - v0) / s32) * f32(SUB))  # float32 throughout, every operation rounded on its own
        assert sub.dtype == f32
        for a in range(3):
            total[s][a] += int(np.clip(sub[:, a].astype(np.int64), 0, top[a]).sum())
    points = cnt[kept].astype(np.int32)
    centroid = np.zeros((S, 3), f32)
    for s in range(S):
        for a in range(3):
            centroid[s, a] = centroid_of(v0[a], s32, total[s][a], points[s])
    out.update(object_labels=np.array([units[r][0] for r in np.flatnonzero(kept)], np.int64).reshape(S), object_points=points,
               object_units=n_units, object_lo=unimage(lo_i).reshape(S, 3), object_hi=unimage(hi_i).reshape(S, 3),
               object_centroid=centroid, n_objects=S, n_units=U, n_components=int(is_root.sum()),
               n_dropped_points=int(cnt[is_root & ~kept].sum()), n_labels=n_labels,
               unit_keys=np.array([key_of(u) for u in units], np.int64), unit_points=upoints, unit_component=root)
    return out
