"""Plain numpy float32 restatement of predict_scene's steps 7a, 8' and 9 ("Labelling a scan"): which chunks
run under a cap, the votes over those chunks only, and the transfer to the points without a vote.  Built on
scene_ref.RefPlan, which restates steps 1-6 and 8; the tests compare the device with this bit for bit."""
import numpy as np

from scene_ref import RefPlan  # noqa: F401  (the plan this file continues)

f32 = np.float32


class RunPlan:
    """Step 7a for a RefPlan p and cap c (None: every chunk runs): run (n_run,) indices into p.chunks, numbered by block id
    then j; run_chunk0 (nb + 1,); run_block (n_run,); slot_map (n_run, N)."""

    def __init__(self, p, cap):
        self.p, self.cap, self.N, self.M = p, cap, p.N, p.M
        self.run, self.run_chunk0 = [], [0]
        for b in range(len(p.block_list)):
            c0, c1 = int(p.block_chunk0[b]), int(p.block_chunk0[b + 1])
            for c in range(c0, c1):
                j = p.chunks[c][1]
                assert j == c - c0
                if cap is None or j < cap:
                    self.run.append(c)
            self.run_chunk0.append(len(self.run))
        self.run = np.array(self.run, np.int64)
        self.n_run, self.n_skipped = len(self.run), p.n_chunks - len(self.run)
        self.run_chunk0 = np.array(self.run_chunk0, np.int32)
        self.run_block = p.chunk_block[self.run].astype(np.int32)
        self.slot_map = p.slot_map[self.run].reshape(self.n_run, p.N)

    def prepared(self, rgb=True, XYZ=True):
        full = self.p.prepared(rgb, XYZ)
        return full[self.run]

    # 8'. an appearance counts when its chunk ran; the order is the one of step 8
    def vote(self, logits):
        """logits (n_run, K, N) float32 -> (scores (M, K) f32, labels (M,) i64, votes (M,) i32)."""
        logits = np.asarray(logits, f32)
        assert logits.shape[0] == self.n_run
        K = logits.shape[1]
        scores, votes = np.zeros((self.M, K), f32), np.zeros(self.M, np.int32)
        for c in range(self.n_run):
            for t in range(self.N):
                q = self.slot_map[c, t]
                scores[q] = scores[q] + logits[c, :, t]
                votes[q] += 1
        labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)
        return scores, labels, votes


def distance(scan, q, p):
    """d of step 9 from point p to the points q (an index array): fp32, every operation rounded on its own."""
    with np.errstate(over="ignore"):
        dx = scan[q, 0] - scan[p, 0]
        dy = scan[q, 1] - scan[p, 1]
        dz = scan[q, 2] - scan[p, 2]
        return ((dx * dx + dy * dy) + dz * dz).astype(f32)


def nearest(scan, q, p, ties=None):
    """The winner among candidates q (scan indices, not empty) for receiver p: the smallest d, then the lowest index.
    ties: a list that collects the receivers for which more than one candidate had that d."""
    d = distance(scan, q, p)
    assert d.dtype == f32 and not np.isnan(d).any()
    best = q[d == d.min()]
    if ties is not None and len(best) > 1:
        ties.append(int(p))
    return int(best.min())


def neighbour_cells(p, key):
    cx, cy = key % p.ncx, key // p.ncx
    return [yy * p.ncx + xx for yy in range(max(cy - 1, 0), min(cy + 1, p.ncy - 1) + 1)
            for xx in range(max(cx - 1, 0), min(cx + 1, p.ncx - 1) + 1)]


# 9. transfer: brute force over the voted points of the 3 x 3 cells
def transfer(p, scores, labels, votes, ties=None):
    """p: RefPlan.  -> (scores, labels, source (M,) i64, n_transferred); the arguments are left unchanged."""
    scores, labels = scores.copy(), labels.copy()
    scan = p.scan
    source = np.where(votes > 0, np.arange(p.M), -1).astype(np.int64)
    voted_of_cell = [np.array([q for q in cell if votes[q] > 0], np.int64) for cell in p.cells]
    n = 0
    for rcv in np.nonzero(p.valid & (votes == 0))[0]:
        cand = [voted_of_cell[c] for c in neighbour_cells(p, int(p.key[rcv]))]
        cand = np.concatenate(cand)
        if len(cand) == 0:
            continue
        q = nearest(scan, cand, rcv, ties)
        source[rcv] = q
        n += 1
    got = (votes == 0) & (source >= 0)
    scores[got] = scores[source[got]]  # sources are voted points: none of them is written
    labels[got] = labels[source[got]]
    return scores, labels, source, n


def transfer_by_cell(p, scores, labels, votes, rows=512):
    """The same result, vectorised per query cell (for cells of thousands of points): a (queries, candidates) matrix of d,
    its row minima, and the lowest index among them."""
    scores, labels = scores.copy(), labels.copy()
    scan = p.scan
    source = np.where(votes > 0, np.arange(p.M), -1).astype(np.int64)
    voted_of_cell = [np.array([q for q in cell if votes[q] > 0], np.int64) for cell in p.cells]
    for key, cell in enumerate(p.cells):
        rcv = np.array([q for q in cell if votes[q] == 0], np.int64)
        cand = np.concatenate([voted_of_cell[c] for c in neighbour_cells(p, key)])
        if len(rcv) == 0 or len(cand) == 0:
            continue
        for r0 in range(0, len(rcv), rows):
            r = rcv[r0:r0 + rows]
            with np.errstate(over="ignore"):
                dx = scan[cand, 0][None, :] - scan[r, 0][:, None]
                dy = scan[cand, 1][None, :] - scan[r, 1][:, None]
                dz = scan[cand, 2][None, :] - scan[r, 2][:, None]
                d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == f32
            tie = d == d.min(1, keepdims=True)
            source[r] = np.where(tie, cand[None, :], np.iinfo(np.int64).max).min(1)
    got = (votes == 0) & (source >= 0)
    scores[got] = scores[source[got]]
    labels[got] = labels[source[got]]
    return scores, labels, source, int(got.sum())


# ---- cases: seeded inputs and their restated results, built once per session; every promise is asserted here -------------
_cache = {}
K = 3
TILES = dict(N=256, stride=1.0, min_points=100, cap=8, M=24000, dense=15000)


def tile_scan():
    """24 000 points on 2 x 2 cells of 1 m, 15 000 of them in cell (1, 1): with N = 256 and cap 8 that cell has more voted
    points than one candidate tile and more points without a vote than one query tile (asserted by the test that knows
    the tile sizes)."""
    if "tile_scan" not in _cache:
        rs = np.random.RandomState(23)
        M, dense = TILES["M"], TILES["dense"]
        xyz = rs.uniform(0.02, 0.98, (M, 3)).astype(f32)
        cell = np.concatenate([np.full(dense, 3), np.arange(M - dense) % 3])
        xyz[:, 0] += (cell % 2).astype(f32)
        xyz[:, 1] += (cell // 2).astype(f32)
        xyz[:, 2] *= f32(3.0)
        xyz[dense, :2], xyz[dense - 1, :2] = (0.0, 0.0), (1.99, 1.99)  # the extent: exactly 2 x 2 cells
        xyz = xyz[rs.permutation(M)]
        _cache["tile_scan"] = np.concatenate([xyz, rs.randint(0, 256, (M, 3)).astype(f32)], 1)
    return _cache["tile_scan"]


def random_logits(n, N, seed):
    return np.random.RandomState(seed).standard_normal((n, K, N)).astype(f32)


class Case:
    """plan p, run plan, seeded logits of the run chunks, the votes of step 8' and the transfer of step 9 on them, and
    what the case exercises (`has`)."""

    def __init__(self, p, cap, seed=0, by_cell=False):
        self.p, self.cap = p, cap
        self.run = RunPlan(p, cap)
        self.logits = random_logits(self.run.n_run, p.N, seed)
        self.scores, self.labels, self.votes = self.run.vote(self.logits)
        ties = []
        if by_cell:
            self.t_scores, self.t_labels, self.source, self.n_transferred = transfer_by_cell(p, self.scores, self.labels, self.votes)
        else:
            self.t_scores, self.t_labels, self.source, self.n_transferred = transfer(p, self.scores, self.labels, self.votes, ties)
        self.n_unlabelled = int((self.t_labels == -1).sum())
        votes, source = self.votes, self.source
        got = (votes == 0) & (source >= 0)
        nc = np.diff(p.block_chunk0)
        in_kept = np.zeros(p.M, bool)
        seen, ran = np.zeros(p.M, np.int32), np.zeros(p.M, np.int32)  # kept blocks holding a point, those it voted through
        for b, lst in enumerate(p.block_list):
            if p.kept[b]:
                in_kept[lst] = True
                seen[lst] += 1
                for c in range(self.run.run_chunk0[b], self.run.run_chunk0[b + 1]):
                    ran[np.unique(self.run.slot_map[c])] += 1
        assert ((ran > 0) == (votes > 0)).all()
        self.has = dict(
            capped=bool((nc > (cap or 10 ** 9)).any()), uncapped=bool(((nc > 0) & (nc <= (cap or 10 ** 9))).any()),
            neighbour=bool((p.key[source[got]] != p.key[got]).any()),
            dropped=bool((got & ~in_kept).any()),
            tie=len(ties) > 0,
            both=bool(((ran > 0) & (ran < seen)).any()),
            no_source=bool((p.valid & (votes == 0) & (source < 0)).any()))


# (scan, r, cap) -> what the case must exercise, asserted when it is built; over the cases every condition occurs
# (conditions_covered): capped and uncapped blocks, a source in a neighbouring cell, a receiver in a dropped block, a tie
# on d decided by the index, a point voted through one block and skipped in another
CASES = {
    "small r=1 c=1": ("small", 1, 1, ("capped", "uncapped", "neighbour", "dropped", "tie")),
    "small r=1 c=2": ("small", 1, 2, ("capped", "uncapped", "neighbour", "dropped", "tie")),
    "small r=2 c=1": ("small", 2, 1, ("capped", "uncapped", "neighbour", "tie", "both")),
    "small r=2 c=2": ("small", 2, 2, ("capped", "uncapped", "both")),  # its few receivers sit beside their sources
    "medium r=2 c=1": ("medium", 2, 1, ("capped", "neighbour", "both")),
}


def case(name):
    import scene_cases as SC
    if name not in _cache:
        which, r, cap, must = CASES[name]
        p = SC.small_plan(r) if which == "small" else SC.medium_plan(r)
        c = Case(p, cap, seed=len(name) + 7 * r + cap)
        missing = [k for k in must if not c.has[k]]
        assert not missing, (name, "the case does not exercise", missing, c.has)
        assert c.run.n_skipped > 0 and c.n_transferred > 0
        _cache[name] = c
    return _cache[name]


def conditions_covered():
    """Every condition the cases are there for occurs in at least one of them."""
    need = {"capped", "uncapped", "neighbour", "dropped", "tie", "both"}
    have = {k for name in CASES for k, v in case(name).has.items() if v}
    assert need <= have, need - have
    return True
