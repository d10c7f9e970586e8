"""The scores of a labelled scan propagated over its occupied-voxel graph: a spatial regulariser between predict_scene and
extract_objects.

predict_scene labels every chunk on its own and sums votes per point, never across points; seams between blocks and isolated
wrong points go into extract_objects as they are, and each becomes an object.  Neighbouring points usually share a class.
The model's head is label propagation over a graph of prototypes; smooth_scene is the same idea at scan scale: the voted
logits are pooled per voxel, swept `iterations` times over the voxel adjacency graph, Z <- (1 - alpha) Y + alpha P Z with P
the row-normalised adjacency, and spread back to the points; a voxel without a voted point is filled from its neighbours ring
by ring.  The reference has no such function, so the behaviour is defined here ("Smoothing a labelled scan",
S1-S7; tests/scene_smooth_ref.py restates it in numpy).  Like the rest of the scene path it draws no random number and adds
no float by an atomic; every fp32 operation and its order are fixed, so the same result and the same scan give the same bits.

  1. valid points, their xyz extent                                               r3d_scene_grow_bounds      host read 1 of 3
  2. voxel keys, stable sort of (key, scan index), voxel heads and their scan     r3d_scene_grow_sort        host read 2 of 3
  3. the voxel table, the voxel of every point, mean colours with colour_tol      r3d_scene_grow_voxels
  4. per voxel the mean of its voted points' mean logits (S2)                     r3d_scene_smooth_evidence
  5. per voxel the rows of its neighbours, ascending (S3)                         r3d_scene_smooth_graph
  6. `iterations` Jacobi sweeps, one launch each (S4)                             r3d_scene_smooth_sweep
  7. voxel labels, every point of a reached voxel takes its row (S5, S6)          r3d_scene_smooth_spread    host read 3 of 3

What alpha means (S7): the sweeps converge to (I - alpha P) Z = (1 - alpha) Y on the voxels with evidence.  A voxel whose
evidence is as strong as its neighbours' cannot be overturned with alpha <= 0.5.  In a synthetic room of 16 x 16 x 8 voxels,
two half-spaces with logits +-1 and 15 % of the voxels flipped (288 of them), alpha = 0.5 changed no label after 2, 4 and
10 sweeps and alpha = 0.8 left 27 to 46 wrong voxels, for both connectivities and 1, 4 and 10 sweeps
(tests/test_scene_smooth_host.py): hence the default.  Nothing is promised about real scans.

This module holds the host logic; the kernels are in csrc/scene_smooth.hip, on the grid and the table of csrc/scene_grow.hip."""
import numpy as np
import torch

from . import ops, scene, scene_grow, scene_segments

MAX_COLS = ops.SCENE_SCORE_COLS_MAX
MAX_ITERATIONS = ops.SCENE_SMOOTH_SWEEPS


class SmoothResult(scene.SceneResult):
    """What smooth_scene returns: a scene.SceneResult, so pool_segments and extract_objects take it as it is.  Per point, on
    the device: labels (M,) int64; scores (M, C) fp32; votes (M,) int32, 1 for a smoothed point, whose row holds MEAN
    logits (a sum over one vote), res.votes for any other; source_votes: res.votes itself; smoothed (M,) bool; voxel_index
    (M,) int32, the row of the point's voxel, -1 for an invalid point.  Per voxel, V rows in ascending key order, on the
    device: voxel_scores (V, C) fp32, the last sweep's Z; voxel_evidence (V, C) fp32, Y; voxel_labels (V,) int64, -1 for a
    voxel never reached; voxel_members (V,) int32, its voted points; voxel_ring (V,) int32, 0 with a member, the sweep that
    filled one without, -1 for one never reached; voxel_means (V, 3) fp32 with colour_tol, else None.  Host ints: n_voxels,
    n_member_voxels, n_filled_voxels, n_smoothed (smoothed points), n_changed (smoothed points with res.labels >= 0 whose
    label differs from it), n_filled (smoothed points whose label in res was -1), n_unlabelled (labels that are -1 in the
    result), n_invalid; grid (nx, ny, nz), (0, 0, 0) without a valid point.  source, neighbours, weights, n_blocks, n_chunks,
    redone, n_transferred, n_chunks_skipped: res's own."""

    def __init__(self, res, **fields):
        super().__init__(fields.pop("labels"), fields.pop("scores"), fields.pop("votes"), res.n_blocks, res.n_chunks,
                         fields.pop("n_unlabelled"), res.redone, source=res.source, n_transferred=res.n_transferred,
                         n_chunks_skipped=res.n_chunks_skipped, neighbours=res.neighbours, weights=res.weights)
        self.source_votes = res.votes
        self.__dict__.update(fields)


def _check_res(res):
    """-> C of a SceneResult whose tensors have the shapes of their class; raises ValueError."""
    if isinstance(res, (scene.SceneSetsResult, scene_segments.SegmentResult)):
        raise ValueError("smooth_scene: res is a %s; only a scene.SceneResult is smoothed (a sets result and a pooled result "
                         "are out of scope)" % type(res).__name__)
    if not isinstance(res, scene.SceneResult):
        raise ValueError("smooth_scene: res must be a scene.SceneResult, got %s" % type(res).__name__)
    sc, votes, labels = res.scores, res.votes, res.labels
    ok = all(isinstance(t, torch.Tensor) for t in (sc, votes, labels)) and sc.dim() == 2 and sc.dtype == torch.float32 and \
        sc.shape[0] >= 1 and sc.shape[1] >= 1 and tuple(votes.shape) == (sc.shape[0],) and votes.dtype == torch.int32 and \
        tuple(labels.shape) == (sc.shape[0],) and labels.dtype == torch.int64
    if not ok:
        raise ValueError("smooth_scene: res does not hold the tensors of a SceneResult (scores (M, n_way + 1) fp32, votes (M,) "
                         "int32, labels (M,) int64)")
    if sc.shape[1] > MAX_COLS:
        raise ValueError("smooth_scene: %d score columns (at most %d)" % (sc.shape[1], MAX_COLS))
    return sc.shape[1]


def check_smooth_args(res, scan, voxel=0.05, connectivity=26, alpha=0.8, iterations=10, colour_tol=None):
    """Raises ValueError before anything needs a device.  -> (C, scan as a tensor, voxel as float32, alpha as float32)."""
    C = _check_res(res)
    scan = scene_grow._check_scan("smooth_scene", scan, 6)
    if scan.shape[0] != res.scores.shape[0]:
        raise ValueError("smooth_scene: a scan of %d points for the %d points of res" % (scan.shape[0], res.scores.shape[0]))
    v32 = scene_grow._check_voxel("smooth_scene", voxel, connectivity, 1)
    a32 = np.float32(alpha) if scene_grow._is_real(alpha) else np.float32(np.nan)
    if not (scene_grow._is_real(alpha) and 0 <= alpha < 1 and a32 < 1):
        raise ValueError("smooth_scene: alpha %r must be a real number in [0, 1) (in float32 too)" % (alpha,))
    if not scene._is_int(iterations) or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError("smooth_scene: iterations %r must be an integer in 0 .. %d" % (iterations, MAX_ITERATIONS))
    scene_grow._check_colour("smooth_scene", colour_tol, scan)
    if not all(t.is_cuda for t in (res.scores, res.votes, res.labels)):  # last: every other refusal comes first on any host
        raise ValueError("smooth_scene: the tensors of res must be on the device")
    return C, scan, v32, a32


def smooth_scene(res, scan, voxel=0.05, connectivity=26, alpha=0.8, iterations=10, colour_tol=None):
    """res: a scene.SceneResult (predict_scene's, with or without a cap or transfer, or built by hand), its tensors on the
    device; scan: the scan it labels, (M, 3) or (M, >= 6) float32, host or device -> SmoothResult.  voxel, connectivity,
    colour_tol: the grid and the graph, as build_segments reads them; alpha in [0, 1): the share of a voxel's row that comes
    from its neighbours in every sweep; iterations 0 .. 64: the sweeps (0: per-voxel pooling alone), each of which also fills
    one more ring of voxels that hold no voted point.  Every valid point of a reached voxel takes the voxel's row and label;
    any other point keeps the bits of res.  res is not modified.  See the module text and INTEGRATION.md, "Smoothing a
    labelled scan"."""
    C, scan, voxel, alpha = check_smooth_args(res, scan, voxel, connectivity, alpha, iterations, colour_tol)
    iterations = int(iterations)
    dev, scan = scene_grow._on_device("smooth_scene", scan, 6, res.scores)
    M = scan.shape[0]
    in_scores, in_votes, in_labels = (t.to(dev).contiguous() for t in (res.scores, res.votes, res.labels))
    ws = ops.scene_grow_workspace(M, dev)
    ops.scene_grow_bounds(scan, ws)
    rec = scene_grow.read_record(ws)  # host read 1 of 3
    n_valid = rec[ops.GROW_R_NVALID]
    if n_valid == 0:  # S1: nothing else is launched
        i32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.int32)
        f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        labels = in_labels.clone()
        return SmoothResult(res, labels=labels, scores=in_scores.clone(), votes=in_votes.clone(),
                            smoothed=torch.zeros(M, device=dev, dtype=torch.bool), voxel_index=torch.full((M,), -1, device=dev, dtype=torch.int32),
                            voxel_scores=f32(0, C), voxel_evidence=f32(0, C), voxel_labels=torch.empty(0, device=dev, dtype=torch.int64),
                            voxel_members=i32(0), voxel_ring=i32(0), voxel_means=f32(0, 3) if colour_tol is not None else None,
                            n_voxels=0, n_member_voxels=0, n_filled_voxels=0, n_smoothed=0, n_changed=0, n_filled=0,
                            n_unlabelled=int((labels == -1).sum()), n_invalid=M, grid=(0, 0, 0))
    lo, hi = scene_grow.extent_of(rec)
    grid = scene_grow.grid_of(lo, hi, voxel, "smooth_scene")
    ops.scene_grow_sort(scan, lo, voxel, grid, ws)
    V = scene_grow.read_record(ws)[ops.GROW_R_V]  # host read 2 of 3
    voxel_index, voxel_means = ops.scene_grow_voxels(scan, grid, n_valid, V, colour_tol is not None, ws)
    evidence, members, ring = ops.scene_smooth_evidence(in_scores, in_votes, grid, V, ws)
    nbr = ops.scene_smooth_graph(M, grid, V, connectivity, voxel_means, colour_tol, ws)
    voxel_scores = ops.scene_smooth_sweep(M, iterations, alpha, evidence, nbr, ring)
    voxel_labels, scores, labels, votes, smoothed, counts = ops.scene_smooth_spread(voxel_index, ring, voxel_scores, in_scores,
                                                                                    in_labels, in_votes)
    n = counts.tolist()  # host read 3 of 3, after everything is queued
    return SmoothResult(res, labels=labels, scores=scores, votes=votes, smoothed=smoothed, voxel_index=voxel_index,
                        voxel_scores=voxel_scores, voxel_evidence=evidence, voxel_labels=voxel_labels, voxel_members=members,
                        voxel_ring=ring, voxel_means=voxel_means, n_voxels=V, n_member_voxels=n[ops.SMOOTH_R_MEMBER_VOXELS],
                        n_filled_voxels=n[ops.SMOOTH_R_FILLED_VOXELS], n_smoothed=n[ops.SMOOTH_R_NSMOOTHED],
                        n_changed=n[ops.SMOOTH_R_NCHANGED], n_filled=n[ops.SMOOTH_R_NFILLED],
                        n_unlabelled=n[ops.SMOOTH_R_NUNLAB], n_invalid=M - n_valid, grid=grid)
