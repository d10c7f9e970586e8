"""Step 10 of predict_scene_sets ("Labelling a scan against several support sets") restated in numpy, one
point and one set at a time: the GPU tests compare r3d_scene_merge_sets with it bit for bit.

  - a point has a label when votes > 0 or (with a transfer) source >= 0; any other point: set_labels -1, labels -1,
    set_of -1, margin 0;
  - per set: l = the arg-max of its n_way + 1 scores, the lowest class on ties, by the comparison of the vote (`v > best`,
    so a NaN never replaces a value and a leading NaN is never replaced);
  - l >= 1 claims the point with m = s[l] - s[r] in fp32, r the arg-max over the other classes by the same comparison;
    a NaN margin does not claim;
  - the greatest margin wins, the lowest set on equal margins: labels = classes[k][l - 1]; no claim: labels = background."""
import numpy as np

f32 = np.float32


def argmax_lowest(s, skip=-1):
    """The vote's arg-max over s without index `skip`: (index, value)."""
    best, best_v = -1, f32(0)
    for j, v in enumerate(s):
        if j != skip and (best < 0 or v > best_v):
            best, best_v = j, v
    return best, best_v


def default_classes(K, n_way):
    return np.arange(K * n_way, dtype=np.int32).reshape(K, n_way)


def merge(scores, votes, source=None, classes=None, background=-1):
    """scores (M, K, C) float32, votes (M,), source (M,) or None, classes (K, C - 1) or None -> (set_labels (M, K) int64,
    labels (M,) int64, set_of (M,) int32, margin (M,) float32)."""
    scores = np.asarray(scores)
    assert scores.dtype == f32 and scores.ndim == 3
    M, K, C = scores.shape
    classes = default_classes(K, C - 1) if classes is None else np.asarray(classes)
    set_labels = np.full((M, K), -1, np.int64)
    labels = np.full(M, -1, np.int64)
    set_of = np.full(M, -1, np.int32)
    margin = np.zeros(M, f32)
    with np.errstate(invalid="ignore"):
        for p in range(M):
            if not (votes[p] > 0 or (source is not None and source[p] >= 0)):
                continue
            win, win_l, win_m = -1, 0, f32(0)
            for k in range(K):
                s = scores[p, k]
                l, lv = argmax_lowest(s)
                set_labels[p, k] = l
                if l < 1:
                    continue
                _, rv = argmax_lowest(s, skip=l)
                m = f32(lv - rv)
                if np.isnan(m):
                    continue
                if win < 0 or m > win_m:
                    win, win_l, win_m = k, l, m
            if win < 0:
                labels[p] = background
            else:
                labels[p], set_of[p], margin[p] = classes[win, win_l - 1], win, win_m
    return set_labels, labels, set_of, margin


def crafted(K, C, M, seed=0):
    """(scores (M, K, C), votes, source) with the rows the definition branches on in front, random rows behind: equal
    margins across sets, ties inside a set (with class 0 and between foreground classes), every set saying background,
    +inf entries (one, and two in a set: a NaN margin), a NaN score, points without a label."""
    rs = np.random.RandomState(seed)
    sc = (rs.randint(-8, 9, (M, K, C)) * f32(0.25)).astype(f32)  # quarters: many exact ties by chance as well
    votes = rs.randint(1, 4, M).astype(np.int32)
    source = np.arange(M, dtype=np.int64)
    top = C - 1
    rows = []

    def row(fill):
        a = np.full((K, C), f32(-1))
        a[:, 0] = 0
        fill(a)
        rows.append(a)
    row(lambda a: a.__setitem__((slice(None), top), f32(1.5)))            # every set claims with the same margin: lowest k
    row(lambda a: (a.__setitem__((0, top), f32(0.5)), a.__setitem__((K - 1, top), f32(2.0))))  # the last set wins
    row(lambda a: a.__setitem__((0, top), f32(0.0)))                      # a tie with class 0: background, no claim
    row(lambda a: a.__setitem__((0, slice(1, None)), f32(3.0)))           # foreground classes tie: lowest class, margin 3 or 0
    row(lambda a: None)                                                   # every set says background
    row(lambda a: a.__setitem__((K - 1, top), f32(np.inf)))               # +inf: an infinite margin wins
    row(lambda a: (a.__setitem__((0, top), f32(np.inf)), a.__setitem__((0, 0), f32(np.inf))))  # inf, inf: class 0 by the tie
    row(lambda a: (a.__setitem__((0, top), f32(np.inf)), a.__setitem__((0, 1), f32(np.inf)), a.__setitem__((0, 0), f32(-np.inf))))
    row(lambda a: (a.__setitem__((0, 0), f32(np.nan)), a.__setitem__((K - 1, top), f32(0.25))))  # a leading NaN stays the best
    row(lambda a: (a.__setitem__((0, top), f32(np.nan)), a.__setitem__((0, 1 if C > 2 else 0), f32(0.5))))
    n = min(len(rows), M)
    sc[:n] = np.stack(rows)[:n]
    # points without a label: no vote and no source; and points a transfer gave a source
    for p in range(n, M, 7):
        votes[p], source[p] = 0, -1
    for p in range(n + 3, M, 11):
        votes[p], source[p] = 0, (p * 5) % M
    return sc, votes, source
