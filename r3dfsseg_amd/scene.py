"""Label a whole scan against a fitted support set.

fit() / predict() take what the reference's episode files hold: clouds of exactly pc_npts points that its loader cut out of
a room, sampled, min-shifted and gave their channels on the host (dataloaders/loader.py:100-119).  predict_scene takes
the scan itself -- (M, 6) rows `x y z r g b`, or (M, 3) for a model without colour -- and returns a label per point.  The
reference has no such function, so the behaviour is defined here ("Labelling a scan"; tests/scene_ref.py
restates it in numpy) and it draws no random number: the same scan gives the same bits.

  1. valid points (finite x, y, z) and their xy extent                       r3d_scene_bounds      host read 1 of 2
  2. cells of `stride` metres, the valid points sorted by cell (stable)      r3d_scene_plan
  3. blocks of r x r cells, r = block_size / stride in 1..4; blocks below
     min_points are dropped; a kept block of n points makes ceil(n / N)
     chunks, chunk j holding list positions j, j + nc, ...                   r3d_scene_plan        host read 2 of 2
  4. per launch, G chunks as prepared clouds of N slots (short chunks wrap)  r3d_scene_prepare
  5. model._predict_groups on them, every chunk its own group (n_q = 1)      what model.predict launches
  6. per scan point the sum of its chunks' logits, in a fixed order          r3d_scene_vote

Two options, both off by default, label a dense scan on an even subsample (steps 7a, 8' and 9 of the definition):
max_chunks_per_block=c runs only chunks j < c of a block (r3d_scene_run_tables; r3d_scene_prepare and r3d_scene_vote then
number the chunks that run; still two host reads), and transfer="nearest" gives every valid point without a vote the
scores and label of the nearest voted point among the 3 x 3 cells around it (r3d_scene_transfer; its count of receivers
is one more host read, at the end); transfer="idw" (step 9') gives it the mean logits of the three nearest such points,
weighted by 1 / (d + 1e-8) with d the squared distance, and the arg-max of those (r3d_scene_transfer given neighbours and
weights: same receivers, same candidates, same host read).  No cap is the cap nobody reaches: every chunk runs.

predict_scene_sets labels the scan against K fitted support sets at once ("Labelling a scan against several
support sets"): steps 1-6 once, per launch one encoder pass and the K heads on its feature rows (step 7s), the vote and the
transfer on logits of K * (n_way + 1) columns, and one merged class id per point (step 10, r3d_scene_merge_sets); per set
the bits of predict_scene.

This module holds the host logic; the kernels are csrc/scene.hip (the sort and the bounds: csrc/scene_sort.hip).  The logits of the chunks that run are kept ((n_chunks,
n_way + 1, N) floats) and summed once at the end; accumulating launch by launch would give the same bits for less memory
and one more pass over the scores per launch."""
import numpy as np
import torch

from . import ops

MAX_CELLS = ops.SCENE_MAX_CELLS
MAX_POINTS = ops.SCENE_MAX_POINTS
TRANSFERS = ("nearest", "idw")
ATTRIBS = {"xyz": (-1, -1), "xyzrgb": (3, -1), "xyzXYZ": (-1, 3), "xyzrgbXYZ": (3, 6)}  # -> (rgb_ch, XYZ_ch)


class SceneResult:
    """labels (M,) int64 in 0..n_way, -1 without a vote; scores (M, n_way + 1) fp32 summed logits; votes (M,) int32 chunk
    slots that held the point -- all on the device; n_blocks (kept), n_chunks (that went through the model), n_unlabelled
    (points whose label is -1), redone: host ints.  With transfer="nearest": source (M,) int64 on the device, the scan index
    a point's label and scores come from (itself with a vote, another point when transferred -- its votes stay 0 --, -1
    without a label), and n_transferred; source is None otherwise.  n_chunks_skipped: chunks a cap left out.
    With transfer="idw": source is the nearest of the neighbours, as with "nearest"; neighbours (M, 3) int64, the scan
    indices q0 q1 q2 a receiver's scores were interpolated from (-1: fewer candidates), (p, -1, -1) for a voted point p, -1
    without a label; weights (M, 3) fp32, their w_i (0 where missing), (1, 0, 0) for a voted point.  A receiver's scores
    are then MEAN logits (every source's sum divided by its votes) while a voted point's stay SUMS over its votes: compare
    scores across the two kinds only after dividing the voted ones by votes.  Both are None otherwise."""

    def __init__(self, labels, scores, votes, n_blocks, n_chunks, n_unlabelled, redone, source=None, n_transferred=0,
                 n_chunks_skipped=0, neighbours=None, weights=None):
        self.labels, self.scores, self.votes = labels, scores, votes
        self.n_blocks, self.n_chunks, self.n_unlabelled, self.redone = n_blocks, n_chunks, n_unlabelled, redone
        self.source, self.n_transferred, self.n_chunks_skipped = source, n_transferred, n_chunks_skipped
        self.neighbours, self.weights = neighbours, weights


def overlap_ratio(block_size, stride):
    """-> (r, s): r = block_size / stride as an integer in 1..4, s = the cell size as fp32."""
    stride = block_size if stride is None else stride
    if not (np.isfinite(block_size) and np.isfinite(stride) and block_size > 0 and stride > 0):
        raise ValueError("predict_scene: block_size %r and stride %r must be positive" % (block_size, stride))
    ratio = float(block_size) / float(stride)
    r = int(round(ratio))
    if r < 1 or r > 4 or abs(ratio - r) > 1e-6 * r:
        raise ValueError("predict_scene: block_size / stride = %r must be an integer in 1..4" % ratio)
    return r, np.float32(stride)


def n_cells_along(lo, hi, s):
    """(int)floorf((hi - lo) / s) + 1 in fp32: the arithmetic the keys kernel applies to every point."""
    return int(np.floor((np.float32(hi) - np.float32(lo)) / np.float32(s))) + 1


def check_sparse_args(max_chunks_per_block, transfer):
    c = max_chunks_per_block
    if c is not None and (isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 1):
        raise ValueError("predict_scene: max_chunks_per_block %r must be None or an integer >= 1" % (c,))
    if transfer is not None and not (isinstance(transfer, str) and transfer in TRANSFERS):
        raise ValueError("predict_scene: transfer %r must be None, \"nearest\" or \"idw\"" % (transfer,))


def check_scene_args(model, scan, block_size, stride, min_points, groups_per_launch, max_chunks_per_block=None, transfer=None):
    """Raises before anything needs a device.  -> (scan as a tensor, r, s, rgb_ch, XYZ_ch)."""
    if model.training:
        raise NotImplementedError("predict_scene is the inference path; call model.eval() first")
    attribs = getattr(model, "pc_attribs", None)
    if attribs not in ATTRIBS or 3 * (1 + sum(c >= 0 for c in ATTRIBS[attribs])) != model.in_channels:
        raise ValueError("predict_scene: a scan cannot supply pc_attribs %r for %d input channels (xyz, then rgb and XYZ if "
                         "present: %s)" % (attribs, model.in_channels, ", ".join(ATTRIBS)))
    rgb_ch, XYZ_ch = ATTRIBS[attribs]
    if isinstance(scan, np.ndarray):
        scan = torch.from_numpy(scan)
    want = 6 if rgb_ch >= 0 else 3
    if not isinstance(scan, torch.Tensor) or scan.dim() != 2 or scan.shape[1] != want or scan.shape[0] < 1:
        raise ValueError("predict_scene: scan must be (M, %d) rows `%s` for pc_attribs %r, got %s"
                         % (want, "x y z r g b" if want == 6 else "x y z", attribs,
                            tuple(scan.shape) if isinstance(scan, torch.Tensor) else type(scan).__name__))
    if scan.dtype != torch.float32:
        raise ValueError("predict_scene: scan must be float32, got %s" % scan.dtype)
    if scan.shape[0] > MAX_POINTS:
        raise ValueError("predict_scene: %d points (at most 2^27)" % scan.shape[0])
    r, s = overlap_ratio(block_size, stride)
    if int(min_points) != min_points or min_points < 1:
        raise ValueError("predict_scene: min_points %r must be an integer >= 1" % (min_points,))
    if int(groups_per_launch) != groups_per_launch or groups_per_launch < 1:
        raise ValueError("predict_scene: groups_per_launch %r must be an integer >= 1" % (groups_per_launch,))
    check_sparse_args(max_chunks_per_block, transfer)
    return scan, r, s, rgb_ch, XYZ_ch


class ScenePlan:
    """Steps 1-5 of the definition for one scan on the device: what r3d_scene_plan left in its workspace, as views.
    order (n_valid,): scan indices sorted by cell, stable; cell_start (n_cells + 1,): offsets of the cells into it;
    block_points (nb,); block_chunk0 (nb + 1,): first chunk of a block; chunk_block (n_chunks,).  Host: x0, y0, xmax,
    ymax (fp32), n_valid, ncx, ncy, nbx, nby, n_chunks, n_blocks (kept).
    The chunks that run (all of them, or with max_chunks_per_block=c those of step 7a): run_chunk0 (nb + 1,): first run
    chunk of a block; run_block (n_run,); host: n_run, n_skipped, n_voted (the valid points of a chunk that runs); prepare
    and vote number the run chunks.  Without a cap the run tables are block_chunk0 and chunk_block themselves, n_run ==
    n_chunks and n_skipped == 0."""

    def __init__(self, scan, N, block_size=1.0, stride=None, min_points=100, max_chunks_per_block=None):
        check_sparse_args(max_chunks_per_block, None)
        if not (scan.is_cuda and scan.dim() == 2 and scan.dtype == torch.float32):
            raise ValueError("ScenePlan: scan must be a (M, ld) float32 tensor on the device")
        self.scan = scan.contiguous()
        self.M, self.N, self.min_points = scan.shape[0], int(N), int(min_points)
        self.r, self.s = overlap_ratio(block_size, stride)
        if self.M > MAX_POINTS:
            raise ValueError("predict_scene: %d points (at most 2^27)" % self.M)
        rec = ops.scene_bounds(self.scan).cpu()  # host read 1 of 2
        self.x0, self.y0, self.xmax, self.ymax = (np.float32(v) for v in rec[:4].tolist())
        self.n_valid = int(rec.view(torch.int32)[4])
        if self.n_valid == 0:
            raise ValueError("predict_scene: the scan has no point with finite x, y and z")
        self.ncx, self.ncy = n_cells_along(self.x0, self.xmax, self.s), n_cells_along(self.y0, self.ymax, self.s)
        if self.ncx * self.ncy > MAX_CELLS:
            raise ValueError("predict_scene: %d x %d cells of %g (at most 65536): use a larger stride or split the scan"
                             % (self.ncx, self.ncy, float(self.s)))
        self.n_cells = self.ncx * self.ncy
        self.nbx, self.nby = max(self.ncx - self.r + 1, 1), max(self.ncy - self.r + 1, 1)
        nb = self.nbx * self.nby
        self.chunk_cap = self.r * self.r * self.n_valid // self.N + nb  # sum of ceil(n_b / N) over blocks never exceeds it
        self.ws, o = ops.scene_workspace(self.M, self.ncx, self.ncy, self.chunk_cap, scan.device)
        ops.scene_plan(self.scan, self.x0, self.y0, self.s, self.ncx, self.ncy, self.r, self.N, self.min_points, self.chunk_cap,
                       self.ws)
        self.cap, self.sws = max_chunks_per_block, None
        self.run_sws = None  # what prepare and vote are given: the run tables, or None for the plan's own chunk tables
        run, run_chunk0, run_block = self.ws, o["block_chunk0"], o["chunk_block"]
        if self.cap is not None:
            run = self.run_sws = self._sparse_workspace()
            run_chunk0, run_block = self.so["run_chunk0"], self.so["run_block"]
            ops.scene_run_tables(self.M, *self._geometry(), min(int(self.cap), 2 ** 30), self.sws)
        rec = self.ws[o["rec"]:o["rec"] + 8].tolist()  # host read 2 of 2
        self.n_chunks, self.n_blocks = rec[:2]
        self.n_run, self.n_skipped, self.n_voted = rec[4:7]
        self.run_chunk0, self.run_block = run[run_chunk0:run_chunk0 + nb + 1], run[run_block:run_block + self.n_run]
        view = lambda name, n: self.ws[o[name]:o[name] + n]
        self.order, self.sorted_key, self.pos = view("order", self.n_valid), view("sorted_key", self.M), view("pos", self.M)
        self.cell_start = view("cell_start", self.n_cells + 1)
        self.block_points, self.block_chunk0 = view("block_points", nb), view("block_chunk0", nb + 1)
        self.chunk_block = view("chunk_block", self.n_chunks)

    def _geometry(self):
        return self.ncx, self.ncy, self.r, self.N, self.chunk_cap, self.ws

    def _sparse_workspace(self):
        if self.sws is None:
            self.sws, self.so = ops.scene_sparse_workspace(self.M, self.ncx, self.ncy, self.chunk_cap, self.scan.device)
        return self.sws

    def prepare(self, first_chunk, out, rgb_ch, XYZ_ch, slot_map=None):
        """Chunks first_chunk .. first_chunk + out.shape[0] - 1 (under a cap: of the chunks that run) as prepared clouds ->
        out (G, C, N), in out's own layout."""
        return ops.scene_prepare(self.scan, *self._geometry(), first_chunk, out, rgb_ch, XYZ_ch, slot_map, sws=self.run_sws)

    def vote(self, logits):
        """logits (n_run, n_classes, N) -> (scores (M, n_classes), labels (M,) int64, votes (M,) int32)."""
        if logits.shape[0] != self.n_run:
            raise ValueError("vote: logits of %d chunks, the plan has %d" % (logits.shape[0], self.n_run))
        if self.n_run == 0:  # every block was dropped: nobody votes
            dev, K = self.scan.device, logits.shape[1]
            return (torch.zeros(self.M, K, device=dev), torch.full((self.M,), -1, device=dev, dtype=torch.int64),
                    torch.zeros(self.M, device=dev, dtype=torch.int32))
        return ops.scene_vote(self.M, *self._geometry(), logits.contiguous(), sws=self.run_sws)

    def transfer(self, scores, labels, votes, mode="nearest"):
        """Step 9 (mode "nearest") or 9' ("idw"), in place on what vote() returned -> (source (M,) int64, n_transferred: a
        (1,) int32 device view), and for "idw" two more: neighbours (M, 3) int64 and weights (M, 3) fp32."""
        if not (isinstance(mode, str) and mode in TRANSFERS):
            raise ValueError("ScenePlan.transfer: mode %r must be \"nearest\" or \"idw\"" % (mode,))
        sws = self._sparse_workspace()
        count = sws[self.so["rec"]:self.so["rec"] + 1]
        args = (self.scan, self.ncx, self.ncy, self.chunk_cap, self.ws, sws, scores, labels, votes)
        if mode == "idw":
            source, neighbours, weights = ops.scene_transfer_idw(*args)
            return source, count, neighbours, weights
        return ops.scene_transfer(*args), count


def staging(G, C, N, device):
    """The reused buffer of G prepared clouds: point-major rows, handed on as the (G, C, N) view the encoder takes as it
    lies (ops.input_layouts: no transpose launch)."""
    return torch.empty(G, N, C, device=device, dtype=torch.float32).transpose(1, 2)


def predict_scene(model, fitted, scan, block_size=1.0, stride=None, min_points=100, groups_per_launch=32, launch=None,
                  max_chunks_per_block=None, transfer=None):
    """model.predict_scene: see the module text.  launch(fitted, query_x (G, 1, C, N)) -> (logits (G, 1, n_way + 1, N),
    redone: bool) runs one launch; the default is the model's own predict launch sequence, the learners pass theirs (MPTI:
    with the redo rule of MPTILearner_V3.predict)."""
    from . import fitted as F
    scan, r, s, rgb_ch, XYZ_ch = check_scene_args(model, scan, block_size, stride, min_points, groups_per_launch,
                                                  max_chunks_per_block, transfer)
    if launch is None:
        launch = lambda f, qx: (model._predict_groups(f, qx, None)[0], False)
    # once: stale fit, shapes, mode -- before the first scene launch
    check = lambda buf: F.check_predict_args(model, fitted, buf[:, None], None)
    plan, scores, labels, votes, redone, source, n_transferred, extra = _voted_scan(
        model, fitted, launch, model.n_way + 1, scan.cuda(), rgb_ch, XYZ_ch, block_size, stride, min_points, groups_per_launch,
        max_chunks_per_block, transfer, check)
    return SceneResult(labels, scores, votes, plan.n_blocks, plan.n_run, plan.M - plan.n_voted - n_transferred, redone,
                       source, n_transferred, plan.n_skipped, *extra)


def _voted_scan(model, fitted, launch, n_cols, scan, rgb_ch, XYZ_ch, block_size, stride, min_points, groups_per_launch,
                max_chunks_per_block, transfer, check=None):
    """Steps 1-9' for a scan on the device, shared by predict_scene and predict_scene_sets: the plan, per launch the
    prepared chunks and launch(fitted, query_x (G, 1, C, N)) -> (logits that reshape to (G, n_cols, N), redone), the vote
    over the (n_run, n_cols, N) logits and the transfer.  -> (plan, scores (M, n_cols), labels, votes, redone, source,
    n_transferred, extra: () or (neighbours, weights))."""
    C, N, K = model.in_channels, model.n_points, n_cols
    G_max = int(groups_per_launch)
    buf = staging(G_max, C, N, scan.device)
    if check is not None:
        check(buf)
    plan = ScenePlan(scan, N, block_size, stride, min_points, max_chunks_per_block)
    logits = torch.empty(plan.n_run, K, N, device=scan.device, dtype=torch.float32)
    redone = 0
    for c0 in range(0, plan.n_run, G_max):
        G = min(G_max, plan.n_run - c0)
        qx = plan.prepare(c0, buf[:G], rgb_ch, XYZ_ch)
        z, again = launch(fitted, qx[:, None])
        redone += bool(again)
        logits[c0:c0 + G].copy_(z.reshape(G, K, N))
    scores, labels, votes = plan.vote(logits)
    source, n_transferred, extra = None, 0, ()
    if transfer is not None:
        source, count, *extra = plan.transfer(scores, labels, votes, transfer)  # "idw": neighbours and weights as well
        n_transferred = int(count.item())  # the one host read the transfer adds, after everything is queued
    return plan, scores, labels, votes, redone, source, n_transferred, tuple(extra)


class SceneSetsResult:
    """What predict_scene_sets returns for K support sets of n_way classes.  On the device: scores (M, K, n_way + 1) fp32 and
    set_labels (M, K) int64 -- [:, k] are the scores and labels predict_scene gives against set k alone, bit for bit --;
    votes (M,) int32, one plan so one count for all sets; labels (M,) int64, the merged class id: classes[k][l - 1] of the
    set k that claims the point with the greatest margin, `background` for a labelled point no set claims, -1 for a point
    without a label (the default background is -1 too: votes and set_labels tell the two apart); set_of (M,) int32, that
    set, or -1; margin (M,) fp32, its margin, 0 where set_of == -1; source, neighbours, weights: as in SceneResult.  Host
    ints with SceneResult's meaning: n_blocks, n_chunks, n_unlabelled (points without a label), redone, n_transferred,
    n_chunks_skipped."""

    def __init__(self, scores, set_labels, votes, labels, set_of, margin, n_blocks, n_chunks, n_unlabelled, redone, source=None,
                 n_transferred=0, n_chunks_skipped=0, neighbours=None, weights=None):
        self.scores, self.set_labels, self.votes = scores, set_labels, votes
        self.labels, self.set_of, self.margin = labels, set_of, margin
        self.n_blocks, self.n_chunks, self.n_unlabelled, self.redone = n_blocks, n_chunks, n_unlabelled, redone
        self.source, self.n_transferred, self.n_chunks_skipped = source, n_transferred, n_chunks_skipped
        self.neighbours, self.weights = neighbours, weights


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_sets_classes(K, n_way, classes, background):
    """-> the (K, n_way) int32 class table of predict_scene_sets (classes None: k * n_way + w - 1); raises ValueError."""
    if not _is_int(background) or not -2 ** 63 <= int(background) < 2 ** 63:
        raise ValueError("predict_scene_sets: background %r must be an integer that fits int64" % (background,))
    if classes is None:
        return np.arange(K * n_way, dtype=np.int32).reshape(K, n_way)
    ok = isinstance(classes, (list, tuple, np.ndarray)) and len(classes) == K and all(
        isinstance(row, (list, tuple, np.ndarray)) and len(row) == n_way and
        all(_is_int(v) and -2 ** 31 <= int(v) < 2 ** 31 for v in row) for row in classes)
    if not ok:
        raise ValueError("predict_scene_sets: classes must be None or %d sequences (one per support set) of n_way = %d "
                         "integers that fit int32, got %r" % (K, n_way, classes))
    return np.array([[int(v) for v in row] for row in classes], dtype=np.int32).reshape(K, n_way)


def predict_scene_sets(model, fits, scan, classes=None, block_size=1.0, stride=None, min_points=100, groups_per_launch=32,
                       launch=None, max_chunks_per_block=None, transfer=None, background=-1):
    """model.predict_scene_sets: one scan against K fitted support sets ("Labelling a scan against several
    support sets").  Steps 1-6, 7a, 8, 8', 9, 9' are predict_scene's, run ONCE: one plan, one staging buffer, every chunk
    prepared once.  Step 7s: per launch of G chunks one encoder pass, then the heads of the K sets on those feature rows;
    the launch's logits lie as (G, K * (n_way + 1), N), set k in columns k * (n_way + 1) .. k * (n_way + 1) + n_way, and the
    vote and the transfer take the (n_run, K * (n_way + 1), N) buffer as it is -- no column of theirs depends on another,
    so set k's scores have the bits predict_scene gives against fits[k].  Step 10: r3d_scene_merge_sets, one label per point.

    launch(fits: fitted.FittedSets, query_x (G, 1, C, N)) -> (logits (G, K * (n_way + 1), N), redone: bool); the default is
    the model's own _predict_groups_sets, the learners pass theirs (MPTI: a launch in which any of the K * G systems missed
    is redone as a whole, as in predict_scene).

    Memory: the logits buffer is K times predict_scene's.  MPTI's head works on E = K * groups_per_launch systems at once
    (ops.HeadBuffers): with n_cap = (n_way + 1) * (n_subprototypes + 1) + n_points and kp1 = k_connect + 1, about
    E * (n_cap * (4 * feat_dim + 32 * planes + 4 * kp1) + 4 * r3d_lp_ws_words(n_cap, kp1)) bytes (node rows, label and
    result rows, the 201-NN lists, the solver's workspace; planes = 1 up to 3 ways, else 2).  Lower groups_per_launch when
    that is too much for the device: it is never lowered silently."""
    from . import fitted as F
    scan, r, s, rgb_ch, XYZ_ch = check_scene_args(model, scan, block_size, stride, min_points, groups_per_launch,
                                                  max_chunks_per_block, transfer)
    fits = F.check_sets_args(model, fits)
    K, C = len(fits), model.n_way + 1
    table = check_sets_classes(K, model.n_way, classes, background)
    if launch is None:
        launch = lambda f, qx: (model._predict_groups_sets(f, qx).reshape(qx.shape[0], K * C, qx.shape[-1]), False)
    scan = scan.cuda()
    plan, scores, _, votes, redone, source, n_transferred, extra = _voted_scan(
        model, fits, launch, K * C, scan, rgb_ch, XYZ_ch, block_size, stride, min_points, groups_per_launch,
        max_chunks_per_block, transfer)
    scores = scores.view(plan.M, K, C)
    set_labels, labels, set_of, margin = ops.scene_merge_sets(scores, votes, source, torch.from_numpy(table).to(scan.device),
                                                              int(background))
    return SceneSetsResult(scores, set_labels, votes, labels, set_of, margin, plan.n_blocks, plan.n_run,
                           plan.M - plan.n_voted - n_transferred, redone, source, n_transferred, plan.n_skipped, *extra)
