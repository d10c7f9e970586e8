"""One label per segment of a labelled scan: pool the scores of predict_scene / predict_scene_sets over user-given segments.

A scan usually comes with a partition of its points -- instance ids, an over-segmentation, supervoxels, the cluster ids of
the reference's loader -- and the last step of a labelling pipeline is one label per segment from the pooled evidence of its
points.  The reference has no such function, so the behaviour is defined here ("Pooling scores over
segments", P1-P5; tests/scene_segments_ref.py restates it in numpy), and like the rest of the scene path it draws no random
number and adds no float by an atomic: the same result and the same segments give the same bits.

  1. the ids: largest legal id, negative ids, ids >= 2^31 - 1 (refused)            r3d_scene_seg_ids    host read 1 of 3
  2. stable sort of (id, scan index), segment rows in ascending id order, the
     contributors (in a segment, votes > 0) of a segment by ascending scan index,
     cut into tiles of 256                                                        r3d_scene_seg_group  host read 2 of 3
  3. per tile the sum of its rows scores / votes, one fp32 addition at a time; per
     segment the sum of its tiles in order, divided by the members; the arg-max     r3d_scene_seg_pool
     (a sets result: r3d_scene_merge_sets on the (S, K, n_way + 1) table, members in the place of votes)
  4. every point of a segment with at least min_members members takes the
     segment's row and label(s); any other point keeps the bits of res            r3d_scene_seg_spread host read 3 of 3

This module holds the host logic; the kernels are in csrc/scene_segments.hip, on the sort of csrc/scene_sort.hip."""
import numpy as np
import torch

from . import ops, scene

MAX_COLS = ops.SCENE_SCORE_COLS_MAX


class SegmentResult:
    """What pool_segments returns.  Per point, on the device: labels (M,) int64; scores (M, n_way + 1), or (M, K, n_way + 1)
    from a sets result, fp32; pooled (M,) bool; segment_index (M,) int32, the row of the point's segment in the tables
    below, -1 for a negative id; votes, source, neighbours, weights: res's own tensors; from a sets result also set_labels
    (M, K) int64, set_of (M,) int32 and margin (M,) fp32 (None otherwise).  A pooled row of scores holds MEAN logits, an
    untouched voted row the SUM over its votes, as res has it: compare the two kinds only after dividing the voted ones
    by votes.
    Per segment, S rows in ascending id order, on the device: segment_ids (S,) int64; segment_points (every point with the
    id) and segment_members (those with a vote) (S,) int32; segment_scores (S, ...) fp32, zeros without a member;
    segment_labels (S,) int64, -1 without a member; from a sets result also segment_set_labels, segment_set_of,
    segment_margin.
    Host ints: n_segments, n_pooled (pooled points), n_filled (pooled points whose label in res was -1), n_unlabelled
    (labels that are -1 in the result)."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _check_res(res):
    """-> (sets: bool, K, C) of a result whose fields have the shapes of their class; raises ValueError."""
    sets = isinstance(res, scene.SceneSetsResult)
    if not sets and not isinstance(res, scene.SceneResult):
        raise ValueError("pool_segments: res must be a scene.SceneResult or a scene.SceneSetsResult, got %s" % type(res).__name__)
    sc, votes, labels = res.scores, res.votes, res.labels
    ok = all(isinstance(t, torch.Tensor) for t in (sc, votes, labels)) and sc.dim() == (3 if sets else 2) and \
        sc.dtype == torch.float32 and sc.shape[0] >= 1 and tuple(votes.shape) == (sc.shape[0],) and votes.dtype == torch.int32 and \
        tuple(labels.shape) == (sc.shape[0],) and labels.dtype == torch.int64
    if ok and sets:
        M, K = sc.shape[:2]
        ok = all(isinstance(t, torch.Tensor) for t in (res.set_labels, res.set_of, res.margin)) and \
            tuple(res.set_labels.shape) == (M, K) and res.set_labels.dtype == torch.int64 and \
            tuple(res.set_of.shape) == (M,) and res.set_of.dtype == torch.int32 and \
            tuple(res.margin.shape) == (M,) and res.margin.dtype == torch.float32 and sc.shape[2] >= 2
    if not ok:
        raise ValueError("pool_segments: res does not hold the tensors of a %s (scores fp32, votes int32, labels int64%s, one "
                         "row per point)" % (type(res).__name__, ", set_labels, set_of, margin" if sets else ""))
    return sets, (sc.shape[1] if sets else 0), sc.shape[-1]


def check_pool_args(res, segments, min_members=1, classes=None, background=-1):
    """Raises ValueError before anything needs a device.  -> (sets, K, C, segments as a tensor, class table or None)."""
    sets, K, C = _check_res(res)
    M = res.scores.shape[0]
    if isinstance(segments, np.ndarray):
        segments = torch.from_numpy(segments)
    if not isinstance(segments, torch.Tensor) or segments.dim() != 1 or segments.dtype not in (torch.int32, torch.int64):
        raise ValueError("pool_segments: segments must be an (M,) int32 or int64 tensor, got %s" % (
            "%s %s" % (tuple(segments.shape), segments.dtype) if isinstance(segments, torch.Tensor) else type(segments).__name__))
    if segments.shape[0] != M:
        raise ValueError("pool_segments: %d segment ids for the %d points of res" % (segments.shape[0], M))
    if M > scene.MAX_POINTS:
        raise ValueError("pool_segments: %d points (at most 2^27)" % M)
    if not scene._is_int(min_members) or min_members < 1:
        raise ValueError("pool_segments: min_members %r must be an integer >= 1" % (min_members,))
    cols = max(K, 1) * C
    if cols > MAX_COLS:
        raise ValueError("pool_segments: %d score columns (at most %d)" % (cols, MAX_COLS))
    table = None
    if sets:
        try:
            table = scene.check_sets_classes(K, C - 1, classes, background)
        except ValueError as e:
            raise ValueError(str(e).replace("predict_scene_sets:", "pool_segments:", 1)) from None
    elif classes is not None or not scene._is_int(background) or background != -1:
        raise ValueError("pool_segments: classes %r and background %r apply to a SceneSetsResult only" % (classes, background))
    return sets, K, C, segments, table


def read_record(ws):
    """The record in front of the workspace as host ints: a host read (the call has three)."""
    return ws[:ops.SCENE_SEG_REC].tolist()


def pool_segments(res, segments, min_members=1, classes=None, background=-1):
    """res: what predict_scene or predict_scene_sets returned; segments (M,) int32 or int64 ids, host or device, negative for
    a point in no segment, else 0 .. 2^31 - 2, neither dense nor sorted -> SegmentResult: per segment the mean of the mean
    logits of its voted points, summed in ascending scan order in tiles of 256, and its label; every point of a segment
    with at least min_members voted points takes them, every other point keeps what res holds.  classes, background: the
    class table of predict_scene_sets, passed again for a SceneSetsResult (the result does not keep it).  res is not
    modified.  See the module text and INTEGRATION.md, "Pooling scores over segments"."""
    sets, K, C, segments, table = check_pool_args(res, segments, min_members, classes, background)
    fields = (res.scores, res.votes, res.labels) + ((res.set_labels, res.set_of, res.margin) if sets else ())
    if not all(t.is_cuda for t in fields):
        raise ValueError("pool_segments: the tensors of res must be on the device")
    dev = res.scores.device
    M, cols = res.scores.shape[0], max(K, 1) * C
    segments = segments.to(dev).contiguous()
    scores_in, votes = res.scores.contiguous().view(M, cols), res.votes.contiguous()
    ws = ops.scene_seg_workspace(M, dev)
    ops.scene_seg_ids(segments, ws)
    rec = read_record(ws)  # host read 1 of 3
    if rec[ops.SEG_R_NBAD] > 0:
        worst = (rec[ops.SEG_R_BADMAX] & 0xFFFFFFFF) | ((rec[ops.SEG_R_BADMAX + 1] & 0xFFFFFFFF) << 32)
        raise ValueError("pool_segments: %d segment ids are 2^31 - 1 or more (the largest: %d); ids must lie in 0 .. 2^31 - 2"
                         % (rec[ops.SEG_R_NBAD], worst))
    segment_index = ops.scene_seg_group(segments, votes, rec[ops.SEG_R_MAX1] - 1, rec[ops.SEG_R_NNEG], ws)
    rec = read_record(ws)  # host read 2 of 3: the tables' sizes
    S, n_tiles = rec[ops.SEG_R_S], rec[ops.SEG_R_NTILES]
    ids, points, members, seg_scores, seg_labels = ops.scene_seg_pool(scores_in, votes, S, n_tiles, ws, want_labels=not sets)
    seg_sets = (None, None, None)
    if sets:
        if S > 0:
            seg_set_labels, seg_labels, seg_set_of, seg_margin = ops.scene_merge_sets(
                seg_scores.view(S, K, C), members, None, torch.from_numpy(table).to(dev), int(background))
        else:
            seg_set_labels = torch.empty(0, K, device=dev, dtype=torch.int64)
            seg_labels = torch.empty(0, device=dev, dtype=torch.int64)
            seg_set_of = torch.empty(0, device=dev, dtype=torch.int32)
            seg_margin = torch.empty(0, device=dev, dtype=torch.float32)
        seg_sets = (seg_set_labels, seg_set_of, seg_margin)
    in_sets = (res.set_labels.contiguous(), res.set_of.contiguous(), res.margin.contiguous()) if sets else (None, None, None)
    scores, labels, set_labels, set_of, margin, pooled = ops.scene_seg_spread(
        int(min_members), segment_index, members, (seg_scores, seg_labels) + seg_sets,
        (scores_in, res.labels.contiguous()) + in_sets, ws)
    rec = read_record(ws)  # host read 3 of 3, after everything is queued
    shape = (K, C) if sets else (C,)
    return SegmentResult(
        labels=labels, scores=scores.view(M, *shape), pooled=pooled, segment_index=segment_index, votes=res.votes,
        source=res.source, neighbours=res.neighbours, weights=res.weights, set_labels=set_labels, set_of=set_of, margin=margin,
        segment_ids=ids, segment_points=points, segment_members=members, segment_scores=seg_scores.view(S, *shape),
        segment_labels=seg_labels, segment_set_labels=seg_sets[0], segment_set_of=seg_sets[1], segment_margin=seg_sets[2],
        n_segments=S, n_pooled=rec[ops.SEG_R_NPOOLED], n_filled=rec[ops.SEG_R_NFILLED], n_unlabelled=rec[ops.SEG_R_NUNLAB])
