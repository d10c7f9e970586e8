"""match_objects ("Matching objects against ground truth", M1-M8) restated in numpy, one stable sort per step
as the definition has them and no dense P x T matrix: the GPU tests compare the kernels with it on integers, and bit for bit
on pair_iou and the summary.

  M1  with ignore_unannotated a point whose truth id is negative counts as negative in pred too;
  M2  per column the distinct non-negative ids, ascending, are its rows; *_points counts the participating points of a row;
  M3  the class of a row is the label of its point with the lowest scan index; a row is mixed when a point differs;
  M4  a pair is a (p, t) with a point in both, in ascending (p, t); pair_iou = f32(inter) / f32(pp + tp - inter);
  M5  eligible: without labels every pair, with labels the pairs of equal classes;
  M6  pred_best / truth_best: the eligible pair with the greatest pair_iou, the lowest partner row on a tie, -1 without one;
  M7  pair_match: for a pair that is the best of both its rows the number of thresholds (float32) its IoU meets;
  M8  per threshold and class, and over all: tp, fp, fn, precision, recall, f1, sq, pq in float64, NaN for x / 0.

The summary's sums are loops of float64 additions in ascending pair order."""
import math

import numpy as np

f32 = np.float32
ID_LIMIT = 2 ** 31 - 1
NAN = float("nan")
FIELDS = ("tp", "fp", "fn", "precision", "recall", "f1", "sq", "pq")


def rows_of(ids, labels=None):
    """ids (M,) with -1 for a point without a row -> (row ids ascending int64, points per row int32, index (M,) int32,
    classes (rows,) int64 or None, mixed rows)."""
    M = len(ids)
    order = np.argsort(np.where(ids >= 0, ids, ID_LIMIT), kind="stable")  # the one sort of (id, scan index)
    n_in = int((ids >= 0).sum())
    sid = ids[order[:n_in]]
    head = np.ones(n_in, bool)
    head[1:] = sid[1:] != sid[:-1]
    row_of_sorted = np.cumsum(head) - 1
    index = np.full(M, -1, np.int32)
    index[order[:n_in]] = row_of_sorted
    starts = np.flatnonzero(head)
    points = np.diff(np.append(starts, n_in)).astype(np.int32)
    classes, n_mixed = None, 0
    if labels is not None:
        first = order[starts]  # the sort is stable: a run's first point has the lowest scan index
        classes = labels[first].astype(np.int64)
        differs = labels[order[:n_in]] != classes[row_of_sorted]
        n_mixed = len(np.unique(row_of_sorted[differs]))
    return sid[starts].astype(np.int64), points, index, classes, n_mixed


def ratio(a, b):
    return float(a) / float(b) if b else NAN


def summarise(iou, n_pred, n_truth, pred_classes, truth_classes, pair_pred, pair_iou, pair_match):
    groups = ["all"] + ([] if pred_classes is None else sorted(set(pred_classes.tolist()) | set(truth_classes.tolist())))
    out = {}
    for j, tau in enumerate(iou):
        out[tau] = {}
        for c in groups:
            tp, total = 0, 0.0
            for k in range(len(pair_pred)):  # ascending pair order
                if pair_match[k] > j and (c == "all" or pred_classes[pair_pred[k]] == c):
                    tp += 1
                    total = total + float(pair_iou[k])
            n_p = n_pred if c == "all" else int((pred_classes == c).sum())
            n_t = n_truth if c == "all" else int((truth_classes == c).sum())
            fp, fn = n_p - tp, n_t - tp
            out[tau][c] = {"tp": tp, "fp": fp, "fn": fn, "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn),
                           "f1": ratio(2 * tp, 2 * tp + fp + fn), "sq": ratio(total, tp), "pq": ratio(total, tp + 0.5 * fp + 0.5 * fn)}
    return out


def match(pred, truth, pred_labels=None, truth_labels=None, iou=(0.25, 0.5, 0.75), ignore_unannotated=False):
    """-> a dict with the fields of scene_match.ObjectMatch as numpy arrays, ints and the summary."""
    pred, truth = np.asarray(pred).astype(np.int64), np.asarray(truth).astype(np.int64)
    M = len(pred)
    assert pred.shape == truth.shape == (M,) and M >= 1 and (pred_labels is None) == (truth_labels is None)
    n_bad = int((pred >= ID_LIMIT).sum() + (truth >= ID_LIMIT).sum())
    if n_bad:
        raise ValueError("%d object ids are 2^31 - 1 or more (the largest: %d)" % (n_bad, max(pred.max(), truth.max())))
    iou = tuple(sorted(float(v) for v in iou))
    labelled = pred_labels is not None
    ignored = (truth < 0) if ignore_unannotated else np.zeros(M, bool)  # M1
    p_ids = np.where(ignored | (pred < 0), -1, pred)
    t_ids = np.where(ignored | (truth < 0), -1, truth)
    out = {"iou": iou, "n_ignored": int(ignored.sum()), "n_pred_unassigned": int((~ignored & (pred < 0)).sum()),
           "n_truth_unassigned": int((~ignored & (truth < 0)).sum())}
    e32, e64 = np.empty(0, np.int32), np.empty(0, np.int64)
    if not (p_ids >= 0).any() or not (t_ids >= 0).any():  # a column without a row: empty tables for both
        none = np.full(M, -1, np.int32)
        cls = e64 if labelled else None
        out.update(pred_ids=e64, pred_points=e32, pred_index=none, pred_classes=cls, pred_best=e32, truth_ids=e64,
                   truth_points=e32, truth_index=none.copy(), truth_classes=cls, truth_best=e32, pair_pred=e32, pair_truth=e32,
                   pair_points=e32, pair_iou=np.empty(0, f32), pair_match=np.empty(0, np.uint8), n_pred=0, n_truth=0, n_pairs=0,
                   n_mixed_pred=0, n_mixed_truth=0,
                   summary=summarise(iou, 0, 0, cls, cls, e32, np.empty(0, f32), np.empty(0, np.uint8)))
        return out
    pl = None if not labelled else np.asarray(pred_labels).astype(np.int64)
    tl = None if not labelled else np.asarray(truth_labels).astype(np.int64)
    pred_ids, pred_points, pred_index, pred_classes, n_mixed_pred = rows_of(p_ids, pl)   # M2, M3
    truth_ids, truth_points, truth_index, truth_classes, n_mixed_truth = rows_of(t_ids, tl)
    P, T = len(pred_ids), len(truth_ids)
    # M4: two stable sorts of 32-bit keys, by truth row, then by the pred row gathered through the first order
    both = (pred_index >= 0) & (truth_index >= 0)
    first = np.argsort(np.where(both, truth_index, T), kind="stable")
    second = first[np.argsort(np.where(both[first], pred_index[first], P), kind="stable")]
    n_both = int(both.sum())
    sp, st = pred_index[second[:n_both]], truth_index[second[:n_both]]
    head = np.ones(n_both, bool)
    head[1:] = (sp[1:] != sp[:-1]) | (st[1:] != st[:-1])
    starts = np.flatnonzero(head)
    pair_pred, pair_truth = sp[starts].astype(np.int32), st[starts].astype(np.int32)
    pair_points = np.diff(np.append(starts, n_both)).astype(np.int32)
    K = len(starts)
    union = pred_points[pair_pred] + truth_points[pair_truth] - pair_points
    pair_iou = pair_points.astype(f32) / union.astype(f32)  # two conversions, one IEEE division
    assert pair_iou.dtype == f32
    eligible = np.ones(K, bool) if not labelled else pred_classes[pair_pred] == truth_classes[pair_truth]  # M5
    pred_best, truth_best = np.full(P, -1, np.int32), np.full(T, -1, np.int32)
    for k in range(K):  # M6: ascending (p, t), so a strict comparison keeps the lowest partner row on a tie
        if not eligible[k]:
            continue
        p, t = pair_pred[k], pair_truth[k]
        if pred_best[p] < 0 or pair_iou[k] > pair_iou[pred_best[p]]:
            pred_best[p] = k
        if truth_best[t] < 0 or pair_iou[k] > pair_iou[truth_best[t]]:
            truth_best[t] = k
    th = np.asarray(iou).astype(f32)
    pair_match = np.zeros(K, np.uint8)
    for k in range(K):  # M7
        if pred_best[pair_pred[k]] == k == truth_best[pair_truth[k]]:
            pair_match[k] = int((pair_iou[k] >= th).sum())
    out.update(pred_ids=pred_ids, pred_points=pred_points, pred_index=pred_index, pred_classes=pred_classes, pred_best=pred_best,
               truth_ids=truth_ids, truth_points=truth_points, truth_index=truth_index, truth_classes=truth_classes,
               truth_best=truth_best, pair_pred=pair_pred, pair_truth=pair_truth, pair_points=pair_points, pair_iou=pair_iou,
               pair_match=pair_match, n_pred=P, n_truth=T, n_pairs=K, n_mixed_pred=n_mixed_pred, n_mixed_truth=n_mixed_truth,
               summary=summarise(iou, P, T, pred_classes, truth_classes, pair_pred, pair_iou, pair_match))
    return out


def same_summary(a, b):
    """Two summaries with the same keys in the same order and the same float64 bits (NaN equals NaN)."""
    if list(a) != list(b):
        return False
    for tau in a:
        if list(a[tau]) != list(b[tau]):
            return False
        for c in a[tau]:
            x, y = a[tau][c], b[tau][c]
            if list(x) != list(FIELDS) or list(y) != list(FIELDS):
                return False
            if not all(np.array_equal(np.float64(x[k]).view(np.uint64), np.float64(y[k]).view(np.uint64)) or
                       (math.isnan(x[k]) and math.isnan(y[k])) for k in x):
                return False
    return True
