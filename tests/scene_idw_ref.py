"""Plain numpy float32 restatement of predict_scene's step 9' ("Labelling a scan"): transfer="idw", the
scores of a point without a vote interpolated from the three nearest voted points of the 3 x 3 cells.  Built on
scene_sparse_ref (distance, neighbour_cells, RunPlan, Case), which restates steps 7a, 8' and 9; the tests compare the
device with this bit for bit.  Two forms: a loop over the receivers, and a per-cell vectorised one for cells of thousands
of points."""
import numpy as np

import scene_cases as SC
import scene_sparse_ref as SR
from scene_ref import RefPlan

f32 = np.float32
EPS = f32(1e-8)


def weights_of(d):
    """w = 1.0f / (d + 1e-8f): an fp32 addition and an fp32 division; d = +inf gives 0."""
    d = np.asarray(d, f32)
    with np.errstate(over="ignore"):
        w = f32(1.0) / (d + EPS)
    assert w.dtype == f32
    return w


def interpolate(m, w):
    """Step 4 for one receiver: m (n, K) mean logits of its n = 1..3 neighbours, w (n,) -> (K,) fp32, one operation at a
    time in the order the definition gives."""
    assert m.dtype == f32 and w.dtype == f32 and 1 <= len(w) <= 3
    with np.errstate(over="ignore", invalid="ignore"):
        acc, wsum = w[0] * m[0], w[0]
        for i in range(1, len(w)):
            acc = acc + w[i] * m[i]
            wsum = wsum + w[i]
        out = m[0] if wsum == 0 else acc / wsum
    assert out.dtype == f32
    return out


def _start(p, votes):
    M = p.M
    source = np.where(votes > 0, np.arange(M), -1).astype(np.int64)
    nbr = np.full((M, 3), -1, np.int64)
    nbr[:, 0] = source
    wgt = np.zeros((M, 3), f32)
    wgt[votes > 0, 0] = 1
    voted_of_cell = [np.array([q for q in cell if votes[q] > 0], np.int64) for cell in p.cells]
    return source, nbr, wgt, voted_of_cell


def idw(p, scores, labels, votes, stats=None):
    """p: RefPlan; scores, labels, votes: what step 8' left.  -> (scores, labels, source (M,) i64, n_transferred,
    neighbours (M, 3) i64, weights (M, 3) f32); the arguments are left unchanged.  stats: a dict that collects the
    receivers with a tie on d among the kept ones (tie_in) and with the last kept and the first dropped candidate at equal
    d (tie_edge)."""
    scores, labels = scores.copy(), labels.copy()
    source, nbr, wgt, voted_of_cell = _start(p, votes)
    n_tr = 0
    for rcv in np.nonzero(p.valid & (votes == 0))[0]:
        cand = np.concatenate([voted_of_cell[c] for c in SR.neighbour_cells(p, int(p.key[rcv]))])
        if len(cand) == 0:
            continue
        d = SR.distance(p.scan, cand, rcv)
        assert d.dtype == f32 and not np.isnan(d).any()
        o = np.lexsort((cand, d))  # by d, then by scan index
        n = min(3, len(cand))
        q, dq = cand[o[:n]], d[o[:n]]
        w = weights_of(dq)
        m = (scores[q] / votes[q].astype(f32)[:, None]).astype(f32)
        s = interpolate(m, w)
        scores[rcv], labels[rcv] = s, int(np.argmax(s))
        source[rcv], nbr[rcv, :n], wgt[rcv, :n] = q[0], q, w
        n_tr += 1
        if stats is not None:
            if n > 1 and (dq[:-1] == dq[1:]).any():
                stats.setdefault("tie_in", []).append(int(rcv))
            if len(cand) > n and d[o[n]] == dq[-1]:
                stats.setdefault("tie_edge", []).append(int(rcv))
    return scores, labels, source, n_tr, nbr, wgt


def idw_by_cell(p, scores, labels, votes, rows=256, stats=None):
    """The same result, vectorised per query cell: a (queries, candidates) matrix of d, then three times the lexicographic
    minimum of (d, index) among the candidates not yet taken."""
    scores, labels = scores.copy(), labels.copy()
    scan = p.scan
    source, nbr, wgt, voted_of_cell = _start(p, votes)
    big = np.iinfo(np.int64).max
    n_tr = 0
    for key, cell in enumerate(p.cells):
        rcv = np.array([q for q in cell if votes[q] == 0], np.int64)
        cand = np.concatenate([voted_of_cell[c] for c in SR.neighbour_cells(p, key)])
        if len(rcv) == 0 or len(cand) == 0:
            continue
        n = min(3, len(cand))
        mean = (scores[cand] / votes[cand].astype(f32)[:, None]).astype(f32)  # (candidates, K)
        for r0 in range(0, len(rcv), rows):
            r = rcv[r0:r0 + rows]
            with np.errstate(over="ignore"):
                dx = scan[cand, 0][None, :] - scan[r, 0][:, None]
                dy = scan[cand, 1][None, :] - scan[r, 1][:, None]
                dz = scan[cand, 2][None, :] - scan[r, 2][:, None]
                d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == f32 and not np.isnan(d).any()
            free = np.ones(d.shape, bool)
            col, dq = np.zeros((len(r), n), np.int64), np.zeros((len(r), n), f32)
            for j in range(n):
                dj = np.where(free, d, f32(np.inf))
                best = dj.min(1, keepdims=True)
                # +inf is a value: a taken candidate is told from a free one at +inf by `free`, not by its d
                qi = np.where(free & (dj == best), cand[None, :], big)
                col[:, j] = qi.argmin(1)
                assert (qi.min(1) < big).all()
                dq[:, j] = d[np.arange(len(r)), col[:, j]]
                free[np.arange(len(r)), col[:, j]] = False
            if stats is not None and len(cand) > n:
                rest = np.where(free, d, f32(np.inf)).min(1)  # len(cand) > n: every row has a free candidate
                stats.setdefault("tie_edge", []).extend(int(x) for x in r[rest == dq[:, -1]])
            if stats is not None and n > 1:
                stats.setdefault("tie_in", []).extend(int(x) for x in r[(dq[:, :-1] == dq[:, 1:]).any(1)])
            w = weights_of(dq)
            with np.errstate(over="ignore", invalid="ignore"):
                acc, wsum = w[:, 0:1] * mean[col[:, 0]], w[:, 0]
                for j in range(1, n):
                    acc = acc + w[:, j:j + 1] * mean[col[:, j]]
                    wsum = wsum + w[:, j]
                s = np.where((wsum == 0)[:, None], mean[col[:, 0]], acc / wsum[:, None])
            assert s.dtype == f32
            scores[r], labels[r] = s, s.argmax(1)
            source[r], nbr[r, :n], wgt[r, :n] = cand[col[:, 0]], cand[col], w
            n_tr += len(r)
    return scores, labels, source, n_tr, nbr, wgt


# ---- cases: a Case of scene_sparse_ref (plan, run plan, seeded logits, votes, the nearest transfer) and step 9' on its votes
_cache = {}
CONDITIONS = ("one", "two", "three", "tie_in", "tie_edge", "zero", "flip", "all_inf", "no_source", "neighbour", "multi_vote")


class IdwCase:
    """c: scene_sparse_ref.Case.  i_scores, i_labels, source, n_transferred, neighbours, weights: step 9' on c's votes;
    `has`: what the case exercises; geometry: what a device plan of the same scan takes."""

    def __init__(self, c, geometry, by_cell=False):
        self.c, self.p, self.geometry = c, c.p, geometry
        p, votes = c.p, c.votes
        stats = {}
        form = idw_by_cell if by_cell else idw
        self.i_scores, self.i_labels, self.source, self.n_transferred, self.neighbours, self.weights = form(
            p, c.scores, c.labels, votes, stats=stats)
        self.n_unlabelled = int((self.i_labels == -1).sum())
        nbr, wgt = self.neighbours, self.weights
        got = (votes == 0) & (self.source >= 0)
        n_nbr = (nbr[got] >= 0).sum(1)
        kept = nbr[got]
        key_q = np.where(kept >= 0, p.key[np.maximum(kept, 0)], p.key[got][:, None])
        d0 = np.array([SR.distance(p.scan, np.array([q]), r)[0] for r, q in zip(np.nonzero(got)[0], nbr[got, 0])], f32)
        self.has = dict(
            one=bool((n_nbr == 1).any()), two=bool((n_nbr == 2).any()), three=bool((n_nbr == 3).any()),
            tie_in=len(stats.get("tie_in", [])) > 0, tie_edge=len(stats.get("tie_edge", [])) > 0,
            zero=bool((d0 == 0).any()),
            flip=bool((self.i_labels[got] != c.labels[self.source[got]]).any()),
            all_inf=bool((np.isinf(d0) & (wgt[got] == 0).all(1)).any()),  # the nearest at +inf, so all of them
            no_source=bool((p.valid & (votes == 0) & (self.source < 0)).any()),
            neighbour=bool((key_q != p.key[got][:, None]).any()),
            multi_vote=bool((votes[kept[kept >= 0]] > 1).any()))
        # what the nearest transfer and step 9' share
        assert np.array_equal(self.source, c.source) and self.n_transferred == c.n_transferred


def _sparse(name):
    which, r, cap, _ = SR.CASES[name]
    par = SC.SMALL if which == "small" else SC.MEDIUM
    scan = SC.small_scan()[0] if which == "small" else SC.medium_scan()
    return IdwCase(SR.case(name), dict(scan=scan, N=par["N"], stride=par["stride"], r=r, min_points=par["min_points"], cap=cap))


def _wide(N, cap):
    scan = SC.wide_scan()
    p = RefPlan(scan, N, block_size=1.0, stride=1.0, min_points=2)
    assert p.n_cells == 65536
    return IdwCase(SR.Case(p, cap, seed=2), dict(scan=scan, N=N, stride=1.0, r=1, min_points=2, cap=cap))


def _tiles():
    T = SR.TILES
    scan = SR.tile_scan()
    p = RefPlan(scan, T["N"], block_size=1.0, stride=1.0, min_points=T["min_points"])
    return IdwCase(SR.Case(p, T["cap"], seed=4, by_cell=True),
                   dict(scan=scan, N=T["N"], stride=T["stride"], r=1, min_points=T["min_points"], cap=T["cap"]), by_cell=True)


ALL_INF_OF = "small r=1 c=1"
FAR_Z = f32(3e19)  # (z_q - 3e19)^2 overflows fp32 for every z_q of the scan


def _all_inf():
    """small r=1 c=1 with the z of one of its receivers at 3e19: z takes no part in cells or list order, so plan and votes
    are those of the case it comes from (asserted), every d of that receiver is +inf and its wsum 0."""
    base = SR.case(ALL_INF_OF)
    _, r, cap, _ = SR.CASES[ALL_INF_OF]
    got = np.nonzero((base.votes == 0) & (base.source >= 0))[0]
    scan = SC.small_scan()[0].copy()
    rcv = int(got[len(got) // 2])
    scan[rcv, 2] = FAR_Z
    p = RefPlan(scan, SC.SMALL["N"], block_size=0.5 * r, stride=0.5, min_points=SC.SMALL["min_points"])
    c = SR.Case(p, cap, seed=len(ALL_INF_OF) + 7 * r + cap)  # the seed scene_sparse_ref.case gives this name
    for a, b in ((p.order, base.p.order), (p.cell_start, base.p.cell_start), (p.slot_map, base.p.slot_map),
                 (c.run.slot_map, base.run.slot_map), (c.logits, base.logits), (c.scores, base.scores), (c.votes, base.votes)):
        assert np.array_equal(a, b)
    case = IdwCase(c, dict(scan=scan, N=SC.SMALL["N"], stride=0.5, r=r, min_points=SC.SMALL["min_points"], cap=cap))
    case.far = rcv
    n = int((case.neighbours[rcv] >= 0).sum())
    assert n >= 1 and (case.weights[rcv] == 0).all() and case.source[rcv] == case.neighbours[rcv, 0]
    assert np.isinf(SR.distance(scan, case.neighbours[rcv, :n], rcv)).all()
    q0 = case.source[rcv]
    assert np.array_equal(case.i_scores[rcv], c.scores[q0] / f32(c.votes[q0]))  # the fallback of step 4
    return case


# name -> (builder, what the case must exercise: asserted when it is built)
CASES = {
    "small r=1 c=1": (lambda: _sparse("small r=1 c=1"), ("three", "tie_in", "tie_edge", "zero", "flip", "neighbour", "multi_vote")),
    "small r=2 c=1": (lambda: _sparse("small r=2 c=1"), ("three", "flip", "neighbour")),
    "medium r=2 c=1": (lambda: _sparse("medium r=2 c=1"), ("three", "flip", "neighbour")),
    "wide N=4": (lambda: _wide(4, None), ("two", "flip", "no_source")),
    "wide N=1 c=1": (lambda: _wide(1, 1), ("one", "two")),
    "tiles": (_tiles, ("three", "flip", "neighbour")),
    "all inf": (_all_inf, ("all_inf", "three", "flip")),
}


def case(name):
    if name not in _cache:
        build, must = CASES[name]
        c = build()
        missing = [k for k in must if not c.has[k]]
        assert not missing, (name, "the case does not exercise", missing, c.has)
        assert c.n_transferred > 0
        _cache[name] = c
    return _cache[name]


def conditions_covered():
    """Every condition the cases are there for occurs in at least one of them."""
    have = {k for name in CASES for k, v in case(name).has.items() if v}
    assert set(CONDITIONS) <= have, set(CONDITIONS) - have
    return True
