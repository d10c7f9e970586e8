"""How good are the objects: a scan's object instances scored against ground-truth instances.

extract_objects, grow_segments and absorb_segments end with one object id per point; a user with ground-truth instance ids
for the same points (the instances column of a block pool, a dataset's annotation, extract_objects on the true labels) asks
how many objects were found.  match_objects answers on the device: per column the distinct ids are ROWS, a PAIR is a pred
row and a truth row that share a point, its IoU is one fp32 division, every row has a BEST partner, and a pair that is the
best of both its rows is a MATCH at every threshold its IoU meets.  Precision, recall, F1, segmentation quality and panoptic
quality per threshold and class follow on the host in float64.  The behaviour is defined here ("Matching
objects against ground truth", M1-M8; tests/scene_match_ref.py restates it in numpy), since the reference scores points only.
Like the rest of the scene path it draws no random number and sends no float through an atomic: the same columns give the
same bits.

  1. per column the largest id and the negatives, the points M1 takes out, ids
     >= 2^31 - 1 (refused)                                                         r3d_scene_match_ids    host read 1 of 4
  2. per column the stable sort of (id, scan index), run heads and their scan, the
     row tables in ascending id order, the row of every point, the mixed rows      r3d_scene_match_rows   host read 2 of 4
  3. ids, points and classes per row; two stable sorts, by truth row and then by
     pred row, heads where (p, t) changes, their scan, the pair tables             r3d_scene_match_pairs  host read 3 of 4
  4. IoU and the eligible flag per pair, truth_best by an integer atomicMax,
     pred_best by a segmented maximum, the mutual best against the thresholds      r3d_scene_match_best
  5. the tables of M8 in one transfer, the summary in float64                                              host read 4 of 4

This module holds the host logic; the kernels are in csrc/scene_match.hip, on the sort and the scan of csrc/scene_sort.hip."""
import numpy as np
import torch

from . import ops, scene

MAX_IOU = ops.SCENE_MATCH_IOU
SUMMARY_FIELDS = ("tp", "fp", "fn", "precision", "recall", "f1", "sq", "pq")


class ObjectMatch:
    """What match_objects returns.  On the device, per column (pred, truth): *_ids (rows,) int64, the distinct non-negative
    ids, ascending; *_points (rows,) int32, the participating points with the id; *_index (M,) int32, the row of the point's
    object, -1 without one; *_classes (rows,) int64, the label of the row's point with the lowest scan index (None without
    labels); *_best (rows,) int32, the pair row of the eligible pair with the greatest IoU, -1 without one.  Per pair, in
    ascending (pred row, truth row): pair_pred, pair_truth, pair_points (n_pairs,) int32 (the intersection), pair_iou
    (n_pairs,) fp32, pair_match (n_pairs,) uint8: how many of the thresholds, in ascending order, a mutual best meets.
    On the host: iou, the thresholds in ascending order; summary: {threshold: {class id or "all": {tp, fp, fn, precision,
    recall, f1, sq, pq}}} (without labels "all" is the only class); ints n_pred (P), n_truth (T), n_pairs,
    n_pred_unassigned, n_truth_unassigned (participating points with a negative id), n_ignored (points M1 took out),
    n_mixed_pred, n_mixed_truth (rows that hold more than one label, 0 without labels)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _check_column(name, t, M=None):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    if not isinstance(t, torch.Tensor) or t.dim() != 1:
        raise ValueError("match_objects: %s must be an (M,) int32 or int64 tensor, got %s" % (
            name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError("match_objects: %s must be int32 or int64, got %s" % (name, t.dtype))
    if M is not None and t.shape[0] != M:
        raise ValueError("match_objects: %d entries in %s for %d points" % (t.shape[0], name, M))
    return t


def check_match_args(pred, truth, pred_labels=None, truth_labels=None, iou=(0.25, 0.5, 0.75), ignore_unannotated=False):
    """Raises ValueError before anything needs a device.  -> (pred, truth, pred_labels, truth_labels as tensors or None, the
    thresholds as a sorted tuple of Python floats, ignore_unannotated as a bool)."""
    pred = _check_column("pred", pred)
    M = pred.shape[0]
    if M < 1 or M > scene.MAX_POINTS:
        raise ValueError("match_objects: %d points (1 .. 2^27)" % M)
    truth = _check_column("truth", truth, M)
    if (pred_labels is None) != (truth_labels is None):
        raise ValueError("match_objects: pred_labels and truth_labels come together or not at all")
    if pred_labels is not None:
        pred_labels, truth_labels = _check_column("pred_labels", pred_labels, M), _check_column("truth_labels", truth_labels, M)
    if not isinstance(iou, (list, tuple, np.ndarray)) or not 1 <= len(iou) <= MAX_IOU:
        raise ValueError("match_objects: iou %r must be a sequence of 1 .. %d thresholds" % (iou, MAX_IOU))
    if not all(isinstance(v, (float, np.floating)) or scene._is_int(v) for v in iou) or \
            not all(0.0 < float(np.float32(v)) <= 1.0 for v in iou):
        raise ValueError("match_objects: iou %r: every threshold must be a number in (0, 1]" % (iou,))
    if not isinstance(ignore_unannotated, (bool, np.bool_)):
        raise ValueError("match_objects: ignore_unannotated %r must be a bool" % (ignore_unannotated,))
    return pred, truth, pred_labels, truth_labels, tuple(sorted(float(v) for v in iou)), bool(ignore_unannotated)


def read_record(ws):
    """The record in front of the workspace as host ints: a host read (the call has four)."""
    return ws[:ops.SCENE_MATCH_REC].tolist()


def read_tables(pred_classes, truth_classes, pair_pred, pair_iou, pair_match):
    """What M8 needs, in ONE transfer: the arrays laid end to end as int32 words on the device, copied once -> (pred_classes,
    truth_classes (None without labels), pair_pred, pair_iou, pair_match) as numpy arrays.  The call's last host read."""
    parts = [pair_pred, pair_iou.view(torch.int32), pair_match.to(torch.int32)]
    if pred_classes is not None:
        parts += [pred_classes.view(torch.int32), truth_classes.view(torch.int32)]
    host = torch.cat(parts).cpu().numpy()
    K = pair_pred.numel()
    pp, iou, match = host[:K], host[K:2 * K].view(np.float32), host[2 * K:3 * K].astype(np.uint8)
    if pred_classes is None:
        return None, None, pp, iou, match
    P = pred_classes.numel()
    return host[3 * K:3 * K + 2 * P].view(np.int64), host[3 * K + 2 * P:].view(np.int64), pp, iou, match


def _ratio(a, b):
    return float(a) / float(b) if b else float("nan")


def summarise(iou, n_pred, n_truth, pred_classes, truth_classes, pair_pred, pair_iou, pair_match):
    """M8, on the host in float64: numpy tables -> {threshold: {class id or "all": {tp, fp, fn, precision, recall, f1, sq,
    pq}}}.  A matched pair has the class of its pred row (equal to its truth row's: M5); sum_iou adds the matches' pair_iou
    in ascending pair order, one float64 addition at a time."""
    groups = [("all", None)]
    if pred_classes is not None:
        groups += [(int(c), int(c)) for c in np.union1d(pred_classes, truth_classes)]
    out = {}
    for j, tau in enumerate(iou):
        rows = np.flatnonzero(pair_match > j)
        cls = pred_classes[pair_pred[rows]] if pred_classes is not None else None
        out[tau] = {}
        for key, c in groups:
            mine = rows if c is None else rows[cls == c]
            n_p = n_pred if c is None else int((pred_classes == c).sum())
            n_t = n_truth if c is None else int((truth_classes == c).sum())
            tp = len(mine)
            total = float(np.cumsum(pair_iou[mine].astype(np.float64))[-1]) if tp else 0.0  # cumsum adds in order
            fp, fn = n_p - tp, n_t - tp
            out[tau][key] = {"tp": tp, "fp": fp, "fn": fn, "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
                             "f1": _ratio(2 * tp, 2 * tp + fp + fn), "sq": _ratio(total, tp),
                             "pq": _ratio(total, tp + 0.5 * fp + 0.5 * fn)}
    return out


def _empty(M, dev, iou, labelled, counts):
    none = torch.full((M,), -1, device=dev, dtype=torch.int32)
    table = lambda dtype: torch.empty(0, device=dev, dtype=dtype)
    e64 = np.empty(0, np.int64)
    classes = lambda: table(torch.int64) if labelled else None
    summary = summarise(iou, 0, 0, e64 if labelled else None, e64 if labelled else None, np.empty(0, np.int32),
                        np.empty(0, np.float32), np.empty(0, np.uint8))
    return ObjectMatch(pred_ids=table(torch.int64), pred_points=table(torch.int32), pred_index=none, pred_classes=classes(),
                       pred_best=table(torch.int32), truth_ids=table(torch.int64), truth_points=table(torch.int32),
                       truth_index=none.clone(), truth_classes=classes(), truth_best=table(torch.int32),
                       pair_pred=table(torch.int32), pair_truth=table(torch.int32), pair_points=table(torch.int32),
                       pair_iou=table(torch.float32), pair_match=table(torch.uint8), iou=iou, summary=summary, n_pred=0, n_truth=0,
                       n_pairs=0, n_mixed_pred=0, n_mixed_truth=0, **counts)


def match_objects(pred, truth, pred_labels=None, truth_labels=None, iou=(0.25, 0.5, 0.75), ignore_unannotated=False):
    """pred, truth (M,) int32 or int64 object ids of the same points, host or device, 1 <= M <= 2^27; negative: the point is
    in no object, else 0 .. 2^31 - 2, neither dense nor sorted (pred is typically SceneObjects.objects or
    GrownSegments.segments) -> ObjectMatch.  pred_labels, truth_labels: both or neither, (M,) int32 or int64 class per point;
    with them only objects of one class are paired.  iou: 1 .. 8 thresholds in (0, 1], compared as float32.
    ignore_unannotated: a point whose truth id is negative takes part in nothing.  A column without a participating
    non-negative id gives empty tables for both.  There is no CPU path.  See the module text and INTEGRATION.md, "Matching
    objects against ground truth"."""
    pred, truth, pred_labels, truth_labels, iou, ignore = check_match_args(pred, truth, pred_labels, truth_labels, iou,
                                                                           ignore_unannotated)
    given = [t for t in (pred, truth, pred_labels, truth_labels) if t is not None]
    on = [t.device for t in given if t.is_cuda]
    if not on and not torch.cuda.is_available():
        raise RuntimeError("match_objects: no device: the matching runs on the GPU, there is no CPU path")
    dev = on[0] if on else torch.device("cuda")
    pred, truth = pred.to(dev).contiguous(), truth.to(dev).contiguous()
    labelled = pred_labels is not None
    if labelled:
        pred_labels, truth_labels = pred_labels.to(dev).contiguous(), truth_labels.to(dev).contiguous()
    M = pred.shape[0]
    ws = ops.scene_match_workspace(M, dev)
    ops.scene_match_ids(pred, truth, ignore, ws)
    rec = read_record(ws)  # host read 1 of 4
    if rec[ops.MATCH_R_NBAD] > 0:
        worst = (rec[ops.MATCH_R_BADMAX] & 0xFFFFFFFF) | ((rec[ops.MATCH_R_BADMAX + 1] & 0xFFFFFFFF) << 32)
        raise ValueError("match_objects: %d object ids are 2^31 - 1 or more (the largest: %d); ids must lie in 0 .. 2^31 - 2"
                         % (rec[ops.MATCH_R_NBAD], worst))
    max1 = rec[ops.MATCH_R_MAX1:ops.MATCH_R_MAX1 + 2]
    n_neg, n_ignored = rec[ops.MATCH_R_NNEG:ops.MATCH_R_NNEG + 2], rec[ops.MATCH_R_NIGNORED]
    counts = dict(n_pred_unassigned=n_neg[0], n_truth_unassigned=n_neg[1], n_ignored=n_ignored)
    if max1[0] == 0 or max1[1] == 0:  # a column without a row: nothing else is launched
        return _empty(M, dev, iou, labelled, counts)
    pred_index, truth_index = ops.scene_match_rows(pred, truth, pred_labels, truth_labels, ignore, (max1[0] - 1, max1[1] - 1),
                                                   (M - n_ignored - n_neg[0], M - n_ignored - n_neg[1]), ws)
    rec = read_record(ws)  # host read 2 of 4: the row tables' sizes
    P, T = rec[ops.MATCH_R_ROWS:ops.MATCH_R_ROWS + 2]
    n_mixed = rec[ops.MATCH_R_MIXED:ops.MATCH_R_MIXED + 2]
    pred_tables, truth_tables = ops.scene_match_pairs(pred_index, truth_index, pred_labels, truth_labels, P, T, ws)
    n_pairs = read_record(ws)[ops.MATCH_R_NPAIRS]  # host read 3 of 4
    pair_pred, pair_truth, pair_points, pair_iou, pred_best, truth_best, pair_match = ops.scene_match_best(
        M, pred_tables, truth_tables, n_pairs, iou, ws)
    host = read_tables(pred_tables[2], truth_tables[2], pair_pred, pair_iou, pair_match)  # host read 4 of 4
    return ObjectMatch(pred_ids=pred_tables[0], pred_points=pred_tables[1], pred_index=pred_index, pred_classes=pred_tables[2],
                       pred_best=pred_best, truth_ids=truth_tables[0], truth_points=truth_tables[1], truth_index=truth_index,
                       truth_classes=truth_tables[2], truth_best=truth_best, pair_pred=pair_pred, pair_truth=pair_truth,
                       pair_points=pair_points, pair_iou=pair_iou, pair_match=pair_match, iou=iou,
                       summary=summarise(iou, P, T, *host), n_pred=P, n_truth=T, n_pairs=n_pairs, n_mixed_pred=n_mixed[0],
                       n_mixed_truth=n_mixed[1], **counts)
