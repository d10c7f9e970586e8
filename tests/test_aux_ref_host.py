"""tests/aux_ref.py against the fp32 oracle (oracle/r3d_oracle.py), on the CPU, and the decidability of every detection
case of tests/test_gpu_aux_kernels.py.

1. decide(box_stats(...)) in float32 gives O.mean_pl_support_y_multi_scale's flags, flag for flag, and its seeds are
   O.grid_sampling's to 1e-6, on every detection case the oracle can run (all but the two with a shot without foreground).
2. similarity(prototypes(pooled(...))) is the head part of O.protonet_forward, both methods.
3. Decidability, for EVERY detection case, way, scale and seed: in float64 every |cs_i - mean(cs)| is at least
   100 x DEV, where DEV is the largest |cs(float32, chain order) - cs(float64)| over all cases; every per-shot share is
   exactly 1/2 by count or off it by at least one seed (half a seed of the doubled count).  The one thing rounding cannot
   move is a way with one or two seeds at a scale: cs = 0, or cs_0 = cs_1 by the symmetry of the product, so cs_i ==
   mean(cs) in every arithmetic -- asserted as an exact identity in float64, float32 and chain-order float32, never as a
   margin.  With the margins asserted here the GPU tests demand the flags exactly.

4. The bars of the GPU tests are 4 x the worst chain-order e32 of their quantity, recomputed here.

Measured over the 22 (case, seed) runs of aux_ref.DETECT_RUNS: DEV = 1.12e-05 (largest chain-order float32 deviation of a
row sum, absolute; the row sums reach 17); smallest margin |cs_i - mean(cs)| in float64 = 1.20e-01 (3w3s-N200-D65-dyadic,
seed 2, way 2, scale (1,1,1)) = 1.08e4 x DEV; 6 per-shot shares are exactly 1/2."""
import numpy as np
import pytest
import torch

import aux_ref as R
from oracle import r3d_oracle as O

F32, F64 = torch.float32, torch.float64
MARGIN_FACTOR = 100.0
_cache = {}
RUN_IDS = ["%s-seed%d" % (R.case_id(c), s) for c, s in R.DETECT_RUNS]


def _case(run):
    """(inputs, {f64, f32, c32: (cnt, box sums, decide(...))}) of a (case, seed)."""
    if run not in _cache:
        c, seed = run
        ref = R.detect_reference(c, seed)
        inp = ref["inp"]
        cnt, bsum = R.box_stats(inp["support_x"], inp["support_y"], inp["feat"], F32)
        _cache[run] = (inp, dict(f64=ref["f64"], c32=ref["c32"], f32=(cnt, bsum, R.decide(cnt, bsum, c[0], c[1], F32))))
    return _cache[run]


def _records(run):
    c = run[0]
    _, st = _case(run)
    for way in range(c[0]):
        for scale in range(2):
            yield way, scale, {k: st[k][2]["rec"][way][scale] for k in st}


@pytest.mark.parametrize("run", [r for r in R.DETECT_RUNS if not R.has_empty_shot(r[0])],
                         ids=[i for i, r in zip(RUN_IDS, R.DETECT_RUNS) if not R.has_empty_shot(r[0])])
def test_detection_restatement_is_the_oracle(run):
    case = run[0]
    n_way, k_shot, N, D, _, Cin = case
    inp, st = _case(run)
    sx = torch.from_numpy(inp["support_x"]).view(n_way, k_shot, Cin, N)
    sy = torch.from_numpy(inp["support_y"]).view(n_way, k_shot, N).long()
    sfeat = torch.from_numpy(inp["feat"]).view(n_way, k_shot, N, D).transpose(2, 3)
    _, want = O.mean_pl_support_y_multi_scale(sfeat, sy, sx)
    got = st["f32"][2]
    assert np.array_equal(got["keep"], want.numpy().astype(np.int64)), (got["keep"], want)
    for scale, n in enumerate((1, 2)):
        _, flag = O.mean_pl_support_y(sfeat, sy, sx, n, n, 1)
        assert np.array_equal(got["flags"][scale], flag.numpy().astype(np.int64)), (scale, got["flags"][scale], flag)
        for way in range(n_way):
            seeds = []
            for k in range(k_shot):
                fg = sy[way, k] == 1
                s, _, _ = O.grid_sampling(sx[way, k][:, fg].t(), sfeat[way, k][:, fg].t(), n, n, 1)
                seeds.append(s)
            seeds = torch.cat(seeds, 0).numpy()
            mine = got["rec"][way][scale]["seeds"]
            assert mine.shape == seeds.shape, (mine.shape, seeds.shape)  # the same boxes came out non-empty
            assert np.abs(mine - seeds).max() <= 1e-6 * max(1.0, np.abs(seeds).max())


@pytest.mark.parametrize("method", ["cosine", "euclidean"])
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_case_id)
def test_head_restatement_is_the_oracle(case, method):
    n_way, k_shot, N, n_q, D, _ = case
    inp = R.head_inputs(case)
    S = n_way * k_shot
    sfeat = torch.from_numpy(inp["sfeat"]).view(n_way, k_shot, N, D).transpose(2, 3)
    qfeat = torch.from_numpy(inp["qfeat"]).view(n_q, N, D).transpose(1, 2)
    sy = torch.from_numpy(inp["support_y"]).view(n_way, k_shot, N).float()
    feats = iter([sfeat.reshape(S, D, N), qfeat])
    real = O.get_features
    O.get_features = lambda sd, x, cfg, *a, **k: next(feats)  # the head part alone: the same features for both
    try:
        cfg = dict(n_way=n_way, k_shot=k_shot, pc_npts=N, pc_in_dim=9)
        want, _ = O.protonet_forward(None, cfg, torch.zeros(S, 9, N), sy, None,
                                     torch.zeros(n_q, N, dtype=torch.long), method)
    finally:
        O.get_features = real
    want = want.transpose(1, 2).reshape(n_q * N, n_way + 1).numpy()
    for dt, bar in ((F32, 1e-6), (F64, 1e-4)):  # the formula itself; then float64 against the oracle's fp32
        P = R.prototypes(R.pooled(inp["sfeat"], inp["support_y"], dt), n_way, k_shot, None, dt)
        got = R.similarity(P, inp["qfeat"], method, 10.0, dt)
        assert got.dtype == R._dt(dt)
        e = R.rel(got, want)
        print("AR| %-28s %-9s %s rel %.2e" % (R.head_case_id(case), method, dt, e))
        assert e <= (bar if case[5] == "unit" or dt == F64 else 1e-4), e


def test_every_detection_case_is_decidable_without_rounding():
    dev, rows = 0.0, []
    for run, rid in zip(R.DETECT_RUNS, RUN_IDS):
        for way, scale, r in _records(run):
            ns = len(r["f64"]["cs"])
            if ns:
                dev = max(dev, float(np.abs(r["c32"]["cs"].astype(np.float64) - r["f64"]["cs"]).max()))
            rows.append((rid, way, scale, ns, r))
    smallest, where = np.inf, None
    ties = 0
    for c, way, scale, ns, r in rows:
        if ns <= 2:  # cs_i == mean(cs) identically: exact in every arithmetic
            for key in ("f64", "f32", "c32"):
                assert ns == 0 or (r[key]["cs"] == r[key]["mean"]).all(), (c, way, scale, key)
            continue
        m = float(np.abs(r["f64"]["cs"] - r["f64"]["mean"]).min())
        if m < smallest:
            smallest, where = m, (c, way, scale)
        pos, tot = r["f64"]["pos"], r["f64"]["tot"]
        ties += int(((2 * pos == tot) & (tot > 0)).sum())
        assert ((2 * pos == tot) | (np.abs(2 * pos - tot) >= 1)).all()
    print("AR| DEV %.3e  smallest margin %.3e at %s  = %.1f x DEV; shares of exactly 1/2: %d" %
          (dev, smallest, where, smallest / dev, ties))
    assert dev < 1e-4, dev  # fp32 rounding of a row sum of <= 32 terms of size <= 1
    assert smallest >= MARGIN_FACTOR * dev, (smallest, dev, where)
    assert ties >= 1  # the `> 0.5` of the vote is exercised by an exact tie
    for run, rid in zip(R.DETECT_RUNS, RUN_IDS):  # and so all three arithmetics take the same decisions
        _, st = _case(run)
        for key in ("f32", "c32"):
            assert np.array_equal(st[key][2]["flags"], st["f64"][2]["flags"]), (rid, key)
            assert np.array_equal(st[key][2]["keep"], st["f64"][2]["keep"])
            assert np.array_equal(st[key][0], st["f64"][0])


def test_the_cases_reach_what_they_are_for():
    """Each property a case is in the table for is there: exact tie of two row sums, empty boxes, points in two boxes, a
    dropped shot, a way reset to all kept, bounds that round below the maximum."""
    seen = dict(two_boxes=0, empty_box=0, dropped=0, reset=0, max_outside=0, tie2=0)
    for run in R.DETECT_RUNS:
        c = run[0]
        inp, st = _case(run)
        cnt, _, dec = st["f64"]
        mem = R.box_members(inp["support_x"], inp["support_y"])
        fgc = (inp["support_y"] == 1).sum(1)
        seen["two_boxes"] += int((mem[:, 1:].sum(1) > 1).sum() > 0 and c[4] == "dyadic")
        seen["empty_box"] += int(((cnt[:, 1:] == 0) & (fgc[:, None] > 0)).any())
        seen["max_outside"] += int((cnt[:, 0] < fgc).any())
        seen["dropped"] += int((dec["keep"] == 0).any())
        seen["reset"] += int(((dec["flags"].sum(0) == 0).all(1)).any())
        seen["tie2"] += int(any(len(dec["rec"][w][0]["cs"]) == 2 for w in range(c[0])))
    print("AR|", seen)
    assert all(v > 0 for k, v in seen.items() if k != "max_outside"), seen


def test_the_bars_of_the_gpu_tests_are_four_times_the_chain_order_e32():
    """tests/test_gpu_aux_kernels.py::BAR, quantity by quantity: 4 x the worst error of the chain-order float32 restatement
    against float64 over that module's cases (to the two digits the table is written in)."""
    import test_gpu_aux_kernels as G
    worst = {}
    for e in [R.detect_e32(c, s) for c, s in R.DETECT_RUNS] + [R.head_e32(c) for c in R.HEAD_CASES]:
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        print("AR| %-8s worst e32 %.3e  x 4 = %.2e  BAR %.1e" % (k, v, 4 * v, G.BAR[k]))
    assert set(worst) == set(G.BAR)
    for k, v in worst.items():
        assert abs(G.BAR[k] / (4 * v) - 1) <= 0.05, (k, v, G.BAR[k])
