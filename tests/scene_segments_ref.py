"""pool_segments ("Pooling scores over segments", P1-P5) restated in numpy, one point and one addition at a
time in fp32: the GPU tests compare the kernels with it bit for bit.

  P1  a point contributes when segments[p] >= 0 and votes[p] > 0; its row is scores[p] / float32(votes[p]);
  P2  the contributors of a segment by ascending scan index;
  P3  ranks in tiles of 256: part = the tile's first row, then += the next ...; tot = the first tile's part, then += the
      next ...; mean = tot / float32(members); no member: zeros;
  P4  the arg-max by the vote's comparison (scene_sets_ref.argmax_lowest), -1 without a member; for a sets result the merge
      of scene_sets_ref on the (S, K, C) table with members in the place of votes;
  P5  a point of a segment with members >= min_members takes its segment's fields, any other point keeps res's.

No float goes through np.sum or a reduceat: every sum is a loop of float32 additions in the stated order (a row is added to
a row element by element, which is the same addition per column)."""
import numpy as np

import scene_sets_ref

f32 = np.float32
TILE = 256


def pool_rows(rows):
    """rows (n, cols) float32, the contributors' rows in rank order, n >= 1 -> tot (cols,) float32 by P3."""
    rows = np.asarray(rows)
    assert rows.dtype == f32 and rows.ndim == 2 and rows.shape[0] >= 1
    tot = None
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, rows.shape[0], TILE):
            part = rows[t0].copy()
            for r in range(t0 + 1, min(t0 + TILE, rows.shape[0])):
                part = part + rows[r]
            tot = part if tot is None else tot + part
    assert tot.dtype == f32
    return tot


def pool(scores, votes, labels, segments, min_members=1, sets=None, classes=None, background=-1):
    """scores (M, cols) or (M, K, C) float32, votes (M,), labels (M,) of res; segments (M,) ints; sets: None, or the
    (set_labels (M, K), set_of (M,), margin (M,)) of a sets result, with classes / background of its merge -> a dict with
    the fields of scene_segments.SegmentResult as numpy arrays and ints."""
    scores = np.asarray(scores)
    assert scores.dtype == f32
    M, shape = scores.shape[0], scores.shape[1:]
    flat = scores.reshape(M, -1)
    cols = flat.shape[1]
    segments = np.asarray(segments).astype(np.int64)
    votes = np.asarray(votes)
    ids = sorted(set(int(g) for g in segments if g >= 0))
    row_of = {g: s for s, g in enumerate(ids)}
    S = len(ids)
    contributors = [[] for _ in range(S)]  # ascending scan index: the loop's order
    points = np.zeros(S, np.int32)
    segment_index = np.full(M, -1, np.int32)
    for p in range(M):
        g = int(segments[p])
        if g < 0:
            continue
        s = row_of[g]
        segment_index[p] = s
        points[s] += 1
        if votes[p] > 0:
            contributors[s].append(p)
    members = np.array([len(c) for c in contributors], np.int32).reshape(S)
    seg_scores = np.zeros((S, cols), f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s, c in enumerate(contributors):
            if c:
                rows = np.stack([flat[p] / f32(votes[p]) for p in c]).astype(f32)
                seg_scores[s] = pool_rows(rows) / f32(len(c))
    out = dict(segment_ids=np.array(ids, np.int64).reshape(S), segment_points=points, segment_members=members,
               segment_scores=seg_scores.reshape((S,) + shape), segment_index=segment_index, n_segments=S)
    if sets is None:
        seg_labels = np.full(S, -1, np.int64)
        with np.errstate(invalid="ignore"):
            for s in range(S):
                if members[s] > 0:
                    seg_labels[s] = scene_sets_ref.argmax_lowest(seg_scores[s])[0]
        seg_sets = None
    else:
        K, C = shape
        if S:
            sl, seg_labels, so, mg = scene_sets_ref.merge(seg_scores.reshape(S, K, C), members, None, classes, background)
        else:
            sl, seg_labels, so, mg = np.zeros((0, K), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, f32)
        seg_sets = (sl, so, mg)
        out.update(segment_set_labels=sl, segment_set_of=so, segment_margin=mg)
    out["segment_labels"] = seg_labels
    new_scores, new_labels = flat.copy(), np.asarray(labels).astype(np.int64).copy()
    pooled = np.zeros(M, bool)
    new_sets = None if sets is None else tuple(np.asarray(a).copy() for a in sets)
    for p in range(M):
        s = segment_index[p]
        if s < 0 or members[s] < min_members:
            continue
        pooled[p] = True
        new_scores[p] = seg_scores[s]
        new_labels[p] = seg_labels[s]
        if new_sets is not None:
            for dst, src in zip(new_sets, seg_sets):
                dst[p] = src[s]
    out.update(scores=new_scores.reshape((M,) + shape), labels=new_labels, pooled=pooled, n_pooled=int(pooled.sum()),
               n_filled=int((pooled & (np.asarray(labels) == -1)).sum()), n_unlabelled=int((new_labels == -1).sum()))
    if new_sets is not None:
        out.update(set_labels=new_sets[0], set_of=new_sets[1], margin=new_sets[2])
    return out


def cancelling_rows(n=257, cols=1):
    """n >= 3 rows 1e8, 1, ..., 1, -1e8, 1: in fp32 the ones vanish beside 1e8, so the sum depends on the order and on the
    tiles (n = 257: 1 by P3, 255 exactly, 0 in reverse)."""
    rows = np.ones((n, cols), f32)
    rows[0] = f32(1e8)
    rows[n - 2] = f32(-1e8)
    return rows
