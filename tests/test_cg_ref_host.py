"""tests/cg_ref.py (the restatement tests/test_gpu_cg_coarse.py compares the coarse-space kernels with) held to its own
algebra and to head_ref.lp_dense's closed form, and every case of tests/cg_cases.py held to the property it was chosen for
and to the preconditions the GPU tests rest on.  No GPU."""
import numpy as np
import pytest
import torch

import cg_cases as CC
import cg_ref as C
import head_ref as R


@pytest.fixture(params=CC.NAMES)
def case(request):
    return CC.get(request.param)


def test_the_graph_is_head_refs(case):
    """cg_ref.graph restates head_ref.lp_from_nodes to keep the degrees: same S, bit for bit; it has the lists' pattern."""
    f = C.reference(case)
    with torch.no_grad():
        S, _ = R.lp_from_nodes(case.x.double(), case.nbr, case.Y, case.sigma, case.alpha)
    assert torch.equal(S, f.S)
    assert torch.equal(f.S != 0, C.pattern(case.nbr))


def test_span_of_W_contains_the_top_mode(case):
    """W 1 = D^1/2 1 exactly (every node lies in one aggregate), and W^T r_0 = 0 to rounding: x_0 = W E^-1 W^T b is the
    Galerkin solution on span(W)."""
    f = C.reference(case)
    assert torch.equal(f.co.W.sum(1), f.co.u) and torch.equal(f.co.u, 1.0 / f.dinv)
    assert torch.equal((f.co.W != 0).sum(1), torch.ones(case.n, dtype=torch.int64))
    b = case.Y.double()
    wr0 = (f.co.W.t() @ f.run.rs[0]).abs().max().item()
    assert wr0 <= 1e-9 * (f.co.W.t() @ b).abs().max().item(), wr0


def test_E_is_spd_on_the_non_empty_aggregates(case):
    f = C.reference(case)
    E, empty = f.co.E, f.co.empty
    assert torch.equal(E, E.t())
    keep = torch.nonzero(~empty).squeeze(1)
    ev = torch.linalg.eigvalsh(E[keep][:, keep])
    assert ev.min().item() > 0
    idx = torch.nonzero(empty).squeeze(1)
    assert (E[idx][:, keep] == 0).all() and torch.equal(E[idx][:, idx], torch.eye(len(idx), dtype=E.dtype))
    assert (f.co.Einv @ E - torch.eye(C.HG_M, dtype=E.dtype)).abs().max().item() < 1e-9


def test_two_level_iterates_reach_the_closed_form(case):
    """Run on to tol 1e-13: the float64 iterates end at head_ref.lp_dense's inv(I - alpha S) Y; the recurrence's residual is
    the true one; the all-zero right-hand-side column stays exactly zero in every iterate."""
    f = C.reference(case)
    with torch.no_grad():
        _, Z, _ = R.lp_dense(case.x, case.nbr, case.Y, case.sigma, case.alpha)
        run = C.two_level_cg(f.co, case.Y, 400, 1e-13)
    assert run.converged == 1 and R.rel(run.xs[-1], Z) <= 1e-8, R.rel(run.xs[-1], Z)
    b = case.Y.double()
    for k in (0, 1, 2, 3, 6, f.run.iters):
        assert (f.run.rs[k] - (b - f.co.M @ f.run.xs[k])).abs().max().item() <= 1e-12 * b.abs().max().item()
    assert (case.Y[:, 3] == 0).all()
    for run_ in (f.run, f.run32, f.plain):
        assert all((x[:, 3] == 0).all() and (r[:, 3] == 0).all() for x, r in zip(run_.xs, run_.rs))


def test_two_level_needs_no_more_iterations_than_plain_cg(case):
    f = C.reference(case)
    for tol in CC.TOLS:
        two, two32, plain = f.count(f.run, tol), f.count(f.run32, tol), f.count(f.plain, tol)
        assert two <= plain, (tol, two, plain)
        if (case.name, tol) not in CC.UNSTABLE:   # (there fp32 has no count of its own: cg_cases.UNSTABLE)
            assert two32 <= plain, (tol, two32, plain)
        if case.prop == "trained":
            assert plain >= 2 * two and plain >= 2 * two32, (tol, two, two32, plain)


def test_preconditions_of_the_gpu_tests(case):
    """What tests/test_gpu_cg_coarse.py takes for granted: no aggregate decision near a tie (fp32 decides as float64 does),
    more than 6 iterations needed, the count not decided on the threshold."""
    f = C.reference(case)
    assert f.gap.min().item() > 1e-4, f.gap.min().item()
    agg32, _ = C.aggregates(case.x, f.src, torch.float32)
    assert torch.equal(agg32, f.agg)
    assert case.n_cap >= case.n + 40
    assert min(f.count(f.run, 1e-6), f.count(f.run32, 1e-6)) > 6
    for T in (1, 2, 3, 6):  # fp32 holds the early iterates themselves well inside the ceiling of the bars
        assert max(C.rel(f.run32.xs[T], f.run.xs[T]), C.rel(f.run32.rs[T], f.run.rs[T])) < 1e-3 / 4, T
    pert = C.perturbed_counts(case, f)
    for i, tol in enumerate(CC.TOLS):
        k, k32 = f.count(f.run, tol), f.count(f.run32, tol)
        off_threshold = f.run.ratio(k, tol) < 0.5 and f.run.ratio(k - 1, tol) > 2.0
        firm = all(p[i] is not None and min(k, k32) <= p[i] <= max(k, k32) for p in pert)
        what = (tol, k, k32, f.run.ratio(k, tol), f.run.ratio(k - 1, tol), sorted({p[i] for p in pert}))
        # float64 decides on which side of the threshold rule a pair falls, the same on every host; what fp32 does is asked
        # only of the pairs held to the window (an fp32 count that one ulp moves is moved by another host's BLAS as well:
        # whether the UNSTABLE pairs show their instability in these eight draws is not asserted)
        assert off_threshold == ((case.name, tol) in CC.COUNT_WINDOW + CC.UNSTABLE), what
        if (case.name, tol) in CC.COUNT_WINDOW:
            assert firm, what


def test_the_property_each_case_was_chosen_for(case):
    f = C.reference(case)
    src, agg, n = f.src, f.agg, case.n
    counts = torch.bincount(agg, minlength=C.HG_M)
    assert int(src[0]) == 0 and int(src[-1]) == max(1, min(case.n_proto, n)) - 1
    if case.prop == "few":
        assert case.n_proto < 64 and len(set(src.tolist())) == min(case.n_proto, 64)
        # a repeated seed row loses every tie to its first copy: exactly the first copies own nodes
        first = [s for s in range(C.HG_M) if s == 0 or src[s] != src[s - 1]]
        assert torch.nonzero(counts).squeeze(1).tolist() == first
        if case.n_proto == 1:
            assert int(f.co.empty.sum()) == 63 and int(counts[0]) == n
    elif case.prop == "edge":
        assert case.n_proto >= 64 and (src[1:] > src[:-1]).all() and (counts > 0).all()
        if case.n_proto == 64:
            assert src.tolist() == list(range(64))
    elif case.prop == "dup":
        assert (src[1:] > src[:-1]).all() and len(case.dup) == 2
        for lo, hi in case.dup:
            assert lo < hi and torch.equal(case.x[src[lo]], case.x[src[hi]]) and counts[hi] == 0 and counts[lo] >= 2
        assert int(f.co.empty.sum()) == 2
    elif case.prop == "chunks":
        rl = C.pattern(case.nbr).sum(1).numpy()
        assert np.array_equal(rl, case.rowlen)
        assert rl[case.A] == 256 and rl[case.B] == 257 and rl[case.hub] == n - 1 and (n - 1 + 255) // 256 == 3
        rest = np.delete(rl, [case.A, case.B, case.hub])
        assert rest.max() <= 16 and rest.min() >= 1
    elif case.prop == "rows":
        assert n % 16 and n % 32 and n % 256
    elif case.prop == "width":
        assert case.D % 4 == 0 and case.D <= 256
    else:
        assert case.prop == "trained"


def test_the_cases_cover_the_table():
    cs = [CC.get(nm) for nm in CC.NAMES]
    assert sorted(c.n_proto for c in cs if c.prop == "few") == [1, 2, 20, 63]
    assert sorted(c.n_proto for c in cs if c.prop == "edge") == [64, 65, 90]
    assert sorted(c.D for c in cs if c.prop == "width") == [4, 64, 132, 252, 256]
    assert sorted(c.n for c in cs if c.prop == "rows") == [31, 33, 255, 257, 513]
    assert {c.prop for c in cs} == {"few", "edge", "dup", "width", "chunks", "rows", "trained"}
    a, b = (CC.get(nm) for nm in CC.BATCH)
    assert a.n != b.n and a.n_proto != b.n_proto and a.D == b.D


def test_seeds_and_ties():
    """The seed formula at its edges, and the tie rule on a hand-made row set."""
    assert C.seeds(1, 10).tolist() == [0] * 64
    assert C.seeds(2, 10).tolist() == [0] * 63 + [1]
    assert C.seeds(64, 100).tolist() == list(range(64))
    assert C.seeds(65, 100).tolist()[-2:] == [62, 64] and C.seeds(65, 100).tolist()[:3] == [0, 1, 2]  # 62.98 -> 62, 64
    assert C.seeds(500, 100).tolist() == C.seeds(100, 100).tolist() and C.seeds(0, 100).tolist() == [0] * 64
    x = torch.zeros(70, 4)
    x[:, 0] = torch.arange(70).float()
    x[5] = x[2]                                     # seed 5 repeats seed 2's row
    agg, gap = C.aggregates(x, C.seeds(64, 70))
    assert agg[2] == 2 and agg[5] == 2 and agg[69] == 63 and agg[64] == 63
    assert gap[2] == 1.0 and abs(gap[69].item() - (49.0 - 36.0) / 49.0) < 1e-12   # node 69: seeds 63 and 62 at 6 and 7
