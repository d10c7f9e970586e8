"""grow_segments, that is build_segments with normal_tol ("Building segments", G3c, G3n and the normal test of G4) restated in numpy:
the GPU tests compare the kernels with it bit for bit.  Every array below is float32 and every numpy call is one rounded
operation; the voxels, the neighbourhood and the summation of a voxel's rows are those of tests/scene_grow_ref.py.

  G3c  u_a = (v_a - v0_a) - float32(i_a) * voxel per point and axis, i from the voxel's key; centroid = the rows u summed by
       scene_segments_ref.pool_rows (tiles of 256, one addition at a time), divided by float32(count);
  G3n  the 27 offsets o = (dz, dy, dx) in lexicographic order over -1, 0, 1; occupied: coordinates inside the grid and the
       voxel in the table; support = their number k; q_o = float32(d) * voxel + centroid[neighbour]; m = the q added one at
       a time by ascending o, divided by float32(k); e_o = q_o - m; C = the six sums of rounded products e e^T by ascending
       o; no normal (NaN row) when k < 4, an entry of C is not finite or max(C00, C11, C22) is not > 0; else B = C / max,
       t = (B00 + B11) + B22, A = t I - B, eight times A <- A A / max(diagonal), normal = the row of A's largest diagonal
       entry (the lowest on a tie);
  G4   c2 = float32(cos(radians(normal_tol)) ** 2); a pair joins when dot * dot >= (c2 * la) * lb -- false with any NaN."""
import math

import numpy as np

import scene_grow_ref as R
import scene_segments_ref

f32 = np.float32
SQUARINGS = 8
MIN_SUPPORT = 4
# o = 0 .. 26 -> (dx, dy, dz): (dz, dy, dx) in lexicographic order, o = 13 the voxel itself
OFFSETS27 = [(o % 3 - 1, (o // 3) % 3 - 1, o // 9 - 1) for o in range(27)]


def cos2_of(normal_tol):
    """The float32 the union compares with: computed in float64, rounded once."""
    return f32(math.cos(math.radians(float(normal_tol))) ** 2)


def centroids(scan, members, vcoord, v0, voxel):
    """G3c.  members: per voxel row the scan indices of its points, ascending; vcoord (V, 3) ints ix iy iz -> (V, 3) float32."""
    s = f32(voxel)
    out = np.zeros((len(members), 3), f32)
    offset = lambda rows, ijk: (scan[rows, :3] - v0) - ijk.astype(f32) * s  # G2's subtraction; a multiplication, a subtraction
    single = np.array([len(m) == 1 for m in members])
    if single.any():  # the sum of one row is the row, and the count is 1
        out[single] = offset(np.array([m[0] for m, one in zip(members, single) if one]), vcoord[single]) / f32(1)
    for v in np.flatnonzero(~single):
        u = offset(members[v], vcoord[v])
        assert u.dtype == f32
        out[v] = scene_segments_ref.pool_rows(np.ascontiguousarray(u)) / f32(len(members[v]))
    return out


def neighbour_rows(vcoord, grid):
    """(V, 27) int64: the row of the occupied voxel at every offset of OFFSETS27, -1 where there is none.  By coordinates."""
    nx, ny, nz = grid
    vcoord = np.asarray(vcoord, np.int64)
    assert (nx + 2) * (ny + 2) * (nz + 2) <= 1 << 26  # a dense array of rows with an empty rim: a lookup by coordinates
    dense = np.full((nz + 2, ny + 2, nx + 2), -1, np.int64)
    dense[vcoord[:, 2] + 1, vcoord[:, 1] + 1, vcoord[:, 0] + 1] = np.arange(len(vcoord))
    return np.stack([dense[vcoord[:, 2] + 1 + dz, vcoord[:, 1] + 1 + dy, vcoord[:, 0] + 1 + dx] for dx, dy, dz in OFFSETS27], 1)


def square(a):
    """N = A A for symmetric A given as [a00, a01, a02, a11, a12, a22], each entry (x y + x' y') + x'' y''."""
    a00, a01, a02, a11, a12, a22 = a
    return [(a00 * a00 + a01 * a01) + a02 * a02,
            (a00 * a01 + a01 * a11) + a02 * a12,
            (a00 * a02 + a01 * a12) + a02 * a22,
            (a01 * a01 + a11 * a11) + a12 * a12,
            (a01 * a02 + a11 * a12) + a12 * a22,
            (a02 * a02 + a12 * a12) + a22 * a22]


def normals_of_cov(C, squarings=SQUARINGS):
    """C (n, 6) float32 rows c00 c01 c02 c11 c12 c22 -> (normals (n, 3) float32, ok (n,) bool): everything of G3n behind C
    but the support; a row without a normal is NaN."""
    C = np.asarray(C)
    assert C.dtype == f32 and C.ndim == 2 and C.shape[1] == 6
    with np.errstate(all="ignore"):
        s = np.maximum(np.maximum(C[:, 0], C[:, 3]), C[:, 5])
        ok = np.isfinite(C).all(1) & (s > 0)
        s = np.where(ok, s, f32(1))
        b = [C[:, i] / s for i in range(6)]
        t = (b[0] + b[3]) + b[5]
        a = [t - b[0], -b[1], -b[2], t - b[3], -b[4], t - b[5]]
        for _ in range(squarings):
            n = square(a)
            mx = np.maximum(np.maximum(n[0], n[3]), n[5])
            a = [x / mx for x in n]
        assert all(x.dtype == f32 for x in a)
        a00, a01, a02, a11, a12, a22 = a
        rows = np.stack([np.stack([a00, a01, a02], 1), np.stack([a01, a11, a12], 1), np.stack([a02, a12, a22], 1)], 1)
        j = np.argmax(np.stack([a00, a11, a22], 1), 1)  # the first of equal maxima
        out = rows[np.arange(len(j)), j]
    out[~ok] = np.nan
    return out, ok


def covariances(cen, nb, voxel):
    """G3n up to C.  cen (V, 3) float32, nb (V, 27) -> (C (V, 6) float32, support (V,) int32)."""
    s = f32(voxel)
    V = len(cen)
    occ = nb >= 0
    k = occ.sum(1).astype(np.int32)
    with np.errstate(all="ignore"):
        q = []
        for o, d in enumerate(OFFSETS27):
            q.append(np.array(d, f32) * s + cen[np.maximum(nb[:, o], 0)])
        m, started = np.zeros((V, 3), f32), np.zeros(V, bool)
        for o in range(27):
            m = np.where((occ[:, o] & ~started)[:, None], q[o], np.where((occ[:, o] & started)[:, None], m + q[o], m))
            started |= occ[:, o]
        m = m / k.astype(f32)[:, None]
        C, started = np.zeros((V, 6), f32), np.zeros(V, bool)
        for o in range(27):
            e = q[o] - m
            p = np.stack([e[:, 0] * e[:, 0], e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 1], e[:, 1] * e[:, 2],
                          e[:, 2] * e[:, 2]], 1)
            C = np.where((occ[:, o] & ~started)[:, None], p, np.where((occ[:, o] & started)[:, None], C + p, C))
            started |= occ[:, o]
    assert m.dtype == f32 and C.dtype == f32
    return C, k


def voxel_normals(cen, nb, voxel):
    """G3n -> (normals (V, 3) float32 with NaN rows, support (V,) int32)."""
    C, k = covariances(cen, nb, voxel)
    n, ok = normals_of_cov(C)
    n[k < MIN_SUPPORT] = np.nan
    return n, k


def alike(na, nb, c2):
    """The normal test of G4 on rows na, nb (..., 3) float32: dot * dot >= (c2 * la) * lb; a NaN makes it False."""
    with np.errstate(all="ignore"):
        dot = (na[..., 0] * nb[..., 0] + na[..., 1] * nb[..., 1]) + na[..., 2] * nb[..., 2]
        la = (na[..., 0] * na[..., 0] + na[..., 1] * na[..., 1]) + na[..., 2] * na[..., 2]
        lb = (nb[..., 0] * nb[..., 0] + nb[..., 1] * nb[..., 1]) + nb[..., 2] * nb[..., 2]
        assert dot.dtype == f32 and la.dtype == f32
        return dot * dot >= (f32(c2) * la) * lb


def grow(scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None, normals=None, cos2=None):
    """-> the dict of scene_grow_ref.grow plus voxel_centroids (V, 3) float32, voxel_normals (V, 3) float32 and voxel_support
    (V,) int32 (None without normal_tol).  normals, cos2: a hand-made table and threshold for the union instead of the scan's
    own (what the tests of the union entry point pass); the centroids and the support stay the scan's."""
    if normal_tol is None and normals is None:
        out = R.grow(scan, voxel, colour_tol, connectivity, min_points)
        out.update(voxel_centroids=None, voxel_normals=None, voxel_support=None)
        return out
    scan = np.asarray(scan)
    M = scan.shape[0]
    valid, v0, coords, (nx, ny, nz) = R.voxels_of(scan, voxel)
    assert max(nx, ny, nz) <= R.MAX_AXIS
    segments, voxel_index = np.full(M, -1, np.int32), np.full(M, -1, np.int32)
    out = dict(segments=segments, voxel_index=voxel_index, segment_points=np.zeros(0, np.int32), n_segments=0, n_voxels=0,
               n_components=0, n_dropped_points=0, n_invalid=int(M - valid.sum()), grid=(nx, ny, nz),
               voxel_means=None if colour_tol is None else np.zeros((0, 3), f32), voxel_centroids=np.zeros((0, 3), f32),
               voxel_normals=np.zeros((0, 3), f32), voxel_support=np.zeros(0, np.int32))
    if not valid.any():
        return out
    keys = (coords[:, 2] * ny + coords[:, 1]) * nx + coords[:, 0]
    vkeys, inverse = np.unique(keys, return_inverse=True)
    V = len(vkeys)
    scan_index = np.flatnonzero(valid)
    voxel_index[scan_index] = inverse.astype(np.int32)
    order = np.argsort(inverse, kind="stable")
    vpoints = np.bincount(inverse, minlength=V).astype(np.int32)
    members = np.split(scan_index[order], np.cumsum(vpoints)[:-1])
    vcoord = np.stack([vkeys % nx, (vkeys // nx) % ny, vkeys // (nx * ny)], 1)
    means = None
    if colour_tol is not None:
        means = np.zeros((V, 3), f32)
        with np.errstate(invalid="ignore", over="ignore"):
            for v, m in enumerate(members):
                means[v] = scene_segments_ref.pool_rows(np.ascontiguousarray(scan[m, 3:6])) / f32(len(m))
    cen = centroids(scan, members, vcoord, v0, voxel)
    nb = neighbour_rows(vcoord, (nx, ny, nz))
    own, support = voxel_normals(cen, nb, voxel)
    table = own if normals is None else np.asarray(normals, f32)
    c2 = cos2_of(normal_tol) if cos2 is None else f32(cos2)
    assert table.shape == (V, 3)
    parent = list(range(V))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    tol = None if colour_tol is None else f32(colour_tol)
    allowed = set(R.offsets(connectivity))
    with np.errstate(invalid="ignore", over="ignore"):
        for o, d in enumerate(OFFSETS27):
            if o <= 13 or d not in allowed:  # every pair once: the offsets behind the voxel itself
                continue
            a = np.flatnonzero(nb[:, o] >= 0)
            b = nb[a, o]
            join = alike(table[a], table[b], c2)
            if tol is not None:
                join &= (np.abs(means[a] - means[b]) <= tol).all(1)  # a NaN joins nothing
            for x, y in zip(a[join].tolist(), b[join].tolist()):
                rx, ry = find(x), find(y)
                if rx != ry:
                    parent[max(rx, ry)] = min(rx, ry)
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
               voxel_component=root, voxel_centroids=cen, voxel_normals=own, voxel_support=support, voxel_coords=vcoord)
    return out
