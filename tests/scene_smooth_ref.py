"""smooth_scene ("Smoothing a labelled scan", S1-S7) restated in numpy, one addition at a time in fp32: the
GPU tests compare the kernels with it bit for bit.

  S1  the grid and the voxel table of build_segments (scene_grow_ref.grow: G1-G3) on the same scan;
  S2  a contributor is a valid point with votes > 0, its row scores[p] / float32(votes[p]); Y[v] = the contributors of voxel v
      by ascending scan index summed by scene_segments_ref.pool_rows (tiles of 256), divided by float32(members); no member:
      zeros;
  S3  the neighbours of v: the occupied voxels among the 6 or 26 cells around it, found by their coordinates in a
      dictionary, that pass the colour test of G4 (with colour_tol), in ascending key order;
  S4  ring_0 = 0 with a member, else -1; Z_0 = Y; sweep t -> t + 1 reads sweep t's arrays only: u is live when 0 <= ring_t[u]
      <= t; n live: s = Z[u_0], s += Z[u_1], ..., m = s / float32(n); a member voxel gets b * Y + a * m, a = float32(alpha), b
      = float32(1) - a; one without gets m and, if its ring is -1, ring = t + 1; n == 0: Z and ring stay;
  S5  voxel_labels: scene_sets_ref.argmax_lowest of the row where ring >= 0, else -1;
  S6  a valid point whose voxel has ring >= 0 takes the voxel's row and label and votes = 1; any other keeps res's.

No float goes through np.sum: every sum is a loop of float32 additions in the stated order."""
import numpy as np

import scene_grow_ref
import scene_segments_ref
import scene_sets_ref

f32 = np.float32


def neighbours_of(grown, connectivity, colour_tol=None):
    """The voxel table of scene_grow_ref.grow -> per voxel the list of its neighbours' rows in ascending key order (S3)."""
    vkeys = grown["voxel_keys"]
    nx, ny, nz = grown["grid"]
    vcoord = np.stack([vkeys % nx, (vkeys // nx) % ny, vkeys // (nx * ny)], 1).tolist()
    row_of = {tuple(c): v for v, c in enumerate(vcoord)}
    means, tol = grown.get("voxel_means"), None if colour_tol is None else f32(colour_tol)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a, (ix, iy, iz) in enumerate(vcoord):
            nb = []
            for dx, dy, dz in scene_grow_ref.offsets(connectivity):  # (dz, dy, dx) lexicographic: ascending key
                b = row_of.get((ix + dx, iy + dy, iz + dz))
                if b is None:
                    continue
                if tol is not None and not bool((np.abs(means[a] - means[b]) <= tol).all()):  # a NaN joins nothing
                    continue
                nb.append(b)
            assert nb == sorted(nb)
            out.append(nb)
    return out


def evidence_of(scores, votes, voxel_index, V):
    """-> (Y (V, C) float32, members (V,) int32) by S2."""
    C = scores.shape[1]
    contributors = [[] for _ in range(V)]
    for p in range(len(voxel_index)):  # ascending scan index
        if voxel_index[p] >= 0 and votes[p] > 0:
            contributors[voxel_index[p]].append(p)
    Y = np.zeros((V, C), f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for v, c in enumerate(contributors):
            if c:
                rows = np.stack([scores[p] / f32(votes[p]) for p in c]).astype(f32)
                Y[v] = scene_segments_ref.pool_rows(rows) / f32(len(c))
    return Y, np.array([len(c) for c in contributors], np.int32).reshape(V)


def sweeps(Y, members, nbrs, alpha, iterations):
    """-> (Z (V, C) float32, ring (V,) int32) after `iterations` sweeps of S4."""
    a = f32(alpha)
    b = f32(1) - a
    Z = Y.copy()
    ring = np.where(members > 0, 0, -1).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(iterations):
            Zn, rn = Z.copy(), ring.copy()
            for v, nb in enumerate(nbrs):
                live = [u for u in nb if 0 <= ring[u] <= t]
                if not live:
                    continue
                s = Z[live[0]].copy()
                for u in live[1:]:
                    s = s + Z[u]
                m = s / f32(len(live))
                if members[v] > 0:
                    Zn[v] = b * Y[v] + a * m
                else:
                    Zn[v] = m
                    if ring[v] < 0:
                        rn[v] = t + 1
            Z, ring = Zn, rn
    assert Z.dtype == f32
    return Z, ring


def smooth(scan, scores, votes, labels, voxel=0.05, connectivity=26, alpha=0.8, iterations=10, colour_tol=None):
    """scan (M, >= 3) float32; scores (M, C) float32, votes (M,), labels (M,) of res -> a dict with the fields of
    scene_smooth.SmoothResult as numpy arrays and ints."""
    scan, scores = np.asarray(scan), np.asarray(scores)
    votes, labels = np.asarray(votes).astype(np.int32), np.asarray(labels).astype(np.int64)
    assert scores.dtype == f32 and scores.ndim == 2
    M, C = scores.shape
    grown = scene_grow_ref.grow(scan, voxel, colour_tol, 6)
    V, voxel_index = grown["n_voxels"], grown["voxel_index"]
    out = dict(scores=scores.copy(), labels=labels.copy(), votes=votes.copy(), source_votes=votes, smoothed=np.zeros(M, bool),
               voxel_index=voxel_index, voxel_scores=np.zeros((0, C), f32), voxel_evidence=np.zeros((0, C), f32),
               voxel_labels=np.zeros(0, np.int64), voxel_members=np.zeros(0, np.int32), voxel_ring=np.zeros(0, np.int32),
               n_voxels=V, n_member_voxels=0, n_filled_voxels=0, n_smoothed=0, n_changed=0, n_filled=0,
               n_unlabelled=int((labels == -1).sum()), n_invalid=grown["n_invalid"], grid=grown["grid"])
    if V == 0:
        return out
    Y, members = evidence_of(scores, votes, voxel_index, V)
    nbrs = neighbours_of(grown, connectivity, colour_tol)
    Z, ring = sweeps(Y, members, nbrs, alpha, iterations)
    voxel_labels = np.full(V, -1, np.int64)
    with np.errstate(invalid="ignore"):
        for v in range(V):
            if ring[v] >= 0:
                voxel_labels[v] = scene_sets_ref.argmax_lowest(Z[v])[0]
    smoothed = (voxel_index >= 0) & (ring[np.maximum(voxel_index, 0)] >= 0)
    new_scores, new_labels, new_votes = out["scores"], out["labels"], out["votes"]
    new_scores[smoothed] = Z[voxel_index[smoothed]]
    new_labels[smoothed] = voxel_labels[voxel_index[smoothed]]
    new_votes[smoothed] = 1
    out.update(smoothed=smoothed, voxel_scores=Z, voxel_evidence=Y, voxel_labels=voxel_labels, voxel_members=members, voxel_ring=ring,
               voxel_means=grown.get("voxel_means"), n_member_voxels=int((ring == 0).sum()), n_filled_voxels=int((ring > 0).sum()),
               n_smoothed=int(smoothed.sum()), n_changed=int((smoothed & (labels >= 0) & (new_labels != labels)).sum()),
               n_filled=int((smoothed & (labels == -1)).sum()), n_unlabelled=int((new_labels == -1).sum()))
    return out
