"""The two-level preconditioner of the label-propagation CG (csrc/head_graph.hip, section 5), stage by stage against
float64: aggregates (r3d_cg_aggregate_kernel), M W (r3d_cg_mw_kernel), E^-1 (r3d_cg_epart_kernel, r3d_cg_einv_kernel) and its
application -- x_0, mu, z -- through the EARLY ITERATES and the ITERATION COUNT (r3d_cg_init_kernel, cg_reduce_step,
r3d_cg_update_kernel and the fused head of r3d_cg_spmv_lds_kernel), through ops.label_propagate and the C ABI.

Why: a wrong preconditioner does not change the converged Z (CG on an SPD system gets there with any reasonable z); it
costs iterations.  An iterate after one to three steps depends on x_0, mu and z to first order.

Reference: tests/cg_ref.py (the definitions of section 5's comment block, dense, float64; held to its own algebra and to
head_ref.lp_dense in tests/test_cg_ref_host.py).  Cases: tests/cg_cases.py, whose preconditions -- no aggregate decision
near a tie, more than 6 iterations needed, counts not decided on the threshold -- are asserted on the host there and again
here where a test rests on them.  Neighbour lists are index decisions made on the host and injected (as
tests/test_gpu_cg_spmv_stream.py does); every case first asserts the CSR the device built against them.

Every call runs with the whole workspace filled with a NaN pattern and NaN in the node rows beyond n, under BOTH SpMV
forms (r3d_debug_set_cg_spmv_lds_min_blocks 0 and 1 << 30), and every compared quantity must have the same bits under the
two.

Bars.  Every figure is max |got - ref64| / max |ref64| (E^-1: max |Einv E64 - I| on the non-empty block -- E is ill
conditioned by design, smallest eigenvalue ~ 1 - alpha, so the residual is judged, not the entries).  Each is printed
beside ``e32``, the same restatement in fp32 on the CPU against float64.  A bar is 4 x the worst figure measured on the
MI355X over this module's cases (the kernels are deterministic: the margin covers other seeds), never above CEIL = 1e-3.
Exact assertions -- aggregates, zeros, symmetry, stats, bit equality -- take no bar.  Measured figures: each test's
docstring and profiles/r33_cg_coarse.md."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cg_cases as CC
import cg_ref as C

pytestmark = pytest.mark.gpu

CEIL = 1e-3
# quantity -> bar = 4 x the worst figure measured over the module's cases (the figures: each test's docstring)
BAR = dict(MW=1.3e-4,     # 3.12e-5 (proto1; e32 1.68e-5)
           Einv=1.3e-5,   # 3.24e-6 (proto20; e32 4.80e-6)
           x1=1.5e-5,     # 3.66e-6 (d252; e32 1.88e-6)
           x2=1.5e-5,     # 3.69e-6 (d252)
           x3=1.5e-5,     # 3.65e-6 (d252)
           x6=1.5e-5,     # 3.68e-6 (d252)
           r1=5.9e-5,     # 1.46e-5 (n33; e32 2.47e-5)
           r2=6.0e-5,     # 1.50e-5 (n33; e32 1.23e-5)
           r3=6.8e-5,     # 1.68e-5 (proto63; e32 2.65e-5)
           r6=1.3e-4,     # 3.23e-5 (dup70; e32 1.45e-5)
           Z=1.5e-5)      # 3.69e-6 (d252; e32 1.81e-6): the converged Z at tol 1e-7
assert max(BAR.values()) <= CEIL
LDS, ROW_PER_WAVE = 0, 1 << 30   # r3d_debug_set_cg_spmv_lds_min_blocks: always / never the LDS form
FORMS = (("lds", LDS), ("rpw", ROW_PER_WAVE))
EARLY = (1, 2, 3, 6)
ITERS = 300
NAN_WORD = 0x7FC00000            # a quiet NaN as fp32, a large positive number as int32
K_SUB = 3                        # HeadBuffers: n_cap = 3 (K_SUB + 1) + n_q_pts


@pytest.fixture(scope="module")
def ops():
    from r3dfsseg_amd import ops as _ops
    from r3dfsseg_amd import _lib
    _lib.load()
    return _ops


def _buffers(ops, n_cap, D, E):
    hb = ops.HeadBuffers(2, 1, 64, n_cap - 3 * (K_SUB + 1), K_SUB, CC.K, D, "cuda", E=E)
    assert hb.n_cap == n_cap and hb.kp1 == CC.K + 1
    return hb


def _load(ops, hb, cases):
    """Node rows beyond n: NaN; lists beyond n: -1."""
    E, nc = hb.E, hb.n_cap
    hb.nodes.fill_(float("nan"))
    hb.Y.zero_()
    nbr = torch.full((E, nc, hb.kp1), -1, dtype=torch.int32)
    for e, c in enumerate(cases):
        hb.nodes[e * nc:e * nc + c.n] = c.x.cuda()
        hb.Y[e * nc:e * nc + c.n] = c.Y.cuda()
        nbr[e, :c.n] = c.nbr.to(torch.int32)
        hb.desc[e, ops.HD_N_PROTO] = c.n_proto
        hb.desc[e, ops.HD_N_NODES] = c.n
    return nbr.cuda().contiguous()


def _call(ops, hb, nbr, cases, min_blocks, max_iter, tol):
    """One r3d_label_propagate_batched with the SpMV form `min_blocks` selects, on a workspace and a Z full of NaN ->
    per system a dict of host tensors (copies)."""
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    nc = hb.n_cap
    old = lib.r3d_debug_set_cg_spmv_lds_min_blocks(min_blocks)
    try:
        hb.lp_ws.fill_(NAN_WORD)
        hb.Z.fill_(float("nan"))
        hb.stats.fill_(-7)
        Z = ops.label_propagate(hb, nbr, CC.SIGMA, CC.ALPHA, max_iter, tol)
        torch.cuda.synchronize()
    finally:
        lib.r3d_debug_set_cg_spmv_lds_min_blocks(old)
    out = []
    for e, c in enumerate(cases):
        agg, MW, Einv, r = hb.coarse(e)
        out.append(dict(Z=Z[e * nc:e * nc + c.n].cpu(), stats=hb.stats[e].cpu(), agg=agg.cpu(), MW=MW.cpu(), Einv=Einv.cpu(),
                        r=r.cpu()))
    return out


def _check_csr(hb, e, c):
    """The CSR the device built has exactly the lists' symmetrised pattern, columns ascending."""
    n_got, row_ptr, col, val = hb.csr(e)
    want = C.pattern(c.nbr)
    assert n_got == c.n
    rows = torch.repeat_interleave(torch.arange(c.n), (row_ptr[1:] - row_ptr[:-1]).cpu())
    want_rc = torch.nonzero(want)  # row-major: rows ascending, columns ascending inside a row
    assert len(rows) == len(want_rc) and torch.equal(rows, want_rc[:, 0]) and torch.equal(col.cpu(), want_rc[:, 1]), \
        "%s: the CSR pattern differs from the lists'" % c.name
    if c.lists == "chunks":
        rl = (row_ptr[1:] - row_ptr[:-1]).cpu().numpy()
        assert rl[c.A] == 256 and rl[c.B] == 257 and rl[c.hub] == c.n - 1 > 512


def _same_bits(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if k == "agg":
            assert torch.equal(x, y), "%s: %s differs" % (what, k)
        else:  # (bitwise, NaN safe: nothing compared may hold a NaN anyway)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "%s: %s differs" % (what, k)


def _runs(ops, hb, nbr, cases):
    """Every call of a set of systems: per form, max_iter = T at tol 1e-6 for T in EARLY, max_iter = 300 at both TOLS."""
    runs = {}
    for form, mb in FORMS:
        for T in EARLY:
            runs[form, "T", T] = _call(ops, hb, nbr, cases, mb, T, 1e-6)
        for tol in CC.TOLS:
            runs[form, "tol", tol] = _call(ops, hb, nbr, cases, mb, ITERS, tol)
    return runs


_solved = {}


@pytest.fixture(params=CC.NAMES)
def sol(request, ops):
    """One case, solved once with every (form, max_iter, tol), the CSR asserted, the two forms held bit for bit."""
    name = request.param
    if name not in _solved:
        c = CC.get(name)
        hb = _buffers(ops, c.n_cap, c.D, 1)
        nbr = _load(ops, hb, [c])
        runs = _runs(ops, hb, nbr, [c])
        _check_csr(hb, 0, c)
        _solved[name] = SimpleNamespace(case=c, runs={k: v[0] for k, v in runs.items()}, ref=C.reference(c), n_cap=hb.n_cap)
    s = _solved[name]
    for key in [k[1:] for k in s.runs if k[0] == "lds"]:
        _same_bits(s.runs[("lds",) + key], s.runs[("rpw",) + key], "%s %s: LDS form against row-per-wave form" % (name, key))
    return s


def _hold(case, errs, e32):
    for k in errs:
        print("CGC| %-8s %-5s err %.2e  e32 %.2e  bar %.1e" % (case, k, errs[k], e32.get(k, float("nan")), BAR[k]))
    bad = {k: v for k, v in errs.items() if not v <= BAR[k]}
    assert not bad, (case, bad)


def _finite(run, n):
    assert all(torch.isfinite(run[k]).all() for k in ("Z", "MW", "Einv")) and torch.isfinite(run["r"][:n]).all()


# ----------------------------------------------------------------------------------------------------------------------
# a. aggregates
# ----------------------------------------------------------------------------------------------------------------------
def test_a_aggregates(sol):
    """agg[:n] is the float64 arg-min over the 64 seed rows for EVERY node (the cases keep every decision more than 1e-4,
    relative, from a tie: asserted here on the host first -- fp32 cannot legitimately choose otherwise), duplicated seed
    rows go to the lower seed, and the same in every call of the case.  agg beyond n is not asserted."""
    c, f = sol.case, sol.ref
    assert f.gap.min().item() > 1e-4
    for key, run in sol.runs.items():
        got = run["agg"]
        assert got.shape == (c.n,) and torch.equal(got, f.agg), \
            "%s %s: %d nodes in another aggregate than the float64 arg-min, first %s" % (
                c.name, key, int((got != f.agg).sum()), torch.nonzero(got != f.agg)[:4].flatten().tolist())
    counts = torch.bincount(sol.runs["lds", "T", 1]["agg"], minlength=C.HG_M)
    for lo, hi in c.dup:
        assert counts[hi] == 0 and counts[lo] > 0
    print("CGC| %-8s aggregates: %d nodes, %d empty, smallest gap %.1e" % (c.name, c.n, int((counts == 0).sum()), f.gap.min().item()))


# ----------------------------------------------------------------------------------------------------------------------
# b. M W
# ----------------------------------------------------------------------------------------------------------------------
def test_b_MW(sol):
    """MW[:n] against float64 (I - alpha S) W built from the DEVICE's aggregates and the float64 S; rows n .. n_cap exactly
    zero; the same bits in every call.
    measured: 3.12e-5 and 2.78e-5 at n_proto = 1 and 2 (e32 1.68e-5 at 1: one or two aggregates, every entry cancels to
    (1 - alpha) u), 5.5e-8 .. 2.3e-7 in the 18 other cases."""
    c, f = sol.case, sol.ref
    run = sol.runs["lds", "T", 1]
    _finite(run, c.n)
    co = C.coarse(f.S, f.dinv, run["agg"], c.alpha)
    assert run["MW"].shape == (sol.n_cap, C.HG_M) and (run["MW"][c.n:] == 0).all(), "rows beyond n are not zero"
    for key, other in sol.runs.items():
        assert torch.equal(other["MW"], run["MW"]) and torch.equal(other["Einv"], run["Einv"]), key
    _hold(c.name, dict(MW=C.rel(run["MW"][:c.n], co.MW)), dict(MW=C.rel(f.co32.MW, f.co.MW)))


# ----------------------------------------------------------------------------------------------------------------------
# c. E^-1
# ----------------------------------------------------------------------------------------------------------------------
def test_c_Einv(sol):
    """Einv is symmetric bit for bit; an empty aggregate a has Einv[a, a] == 1 and an exactly zero rest of its row and
    column; max |Einv E64 - I| on the non-empty block, E64 the float64 coarse operator of the device's aggregates.
    measured: 3.24e-6 at worst (n_proto = 20; e32, an fp32 inverse of the fp32 E, 4.80e-6)."""
    c, f = sol.case, sol.ref
    run = sol.runs["lds", "T", 1]
    Einv = run["Einv"]
    assert torch.equal(Einv, Einv.t()), "E^-1 is not symmetric bit for bit"
    co = C.coarse(f.S, f.dinv, run["agg"], c.alpha)
    empty = torch.nonzero(co.empty).squeeze(1)
    keep = torch.nonzero(~co.empty).squeeze(1)
    assert len(empty) == int(f.co.empty.sum())
    for a in empty.tolist():
        row = Einv[a].clone()
        assert row[a] == 1.0
        row[a] = 0.0
        assert (row == 0).all(), "empty aggregate %d: row / column not zero" % a
    I = torch.eye(len(keep), dtype=torch.float64)
    res = (Einv[keep][:, keep].double() @ co.E[keep][:, keep] - I).abs().max().item()
    res32 = (f.co32.Einv[keep][:, keep].double() @ f.co.E[keep][:, keep] - I).abs().max().item()
    _hold(c.name, dict(Einv=res), dict(Einv=res32))


# ----------------------------------------------------------------------------------------------------------------------
# d. early iterates
# ----------------------------------------------------------------------------------------------------------------------
def test_d_early_iterates(sol):
    """max_iter = T for T in 1, 2, 3, 6 on systems that need more than 6 iterations (asserted in float64 and fp32 on the
    host): stats == {converged 0, iters T}, Z[:n] is the float64 iterate x_T and r in the workspace the float64 residual
    r_T (rows n .. n_cap exactly zero); the all-zero column of the right-hand side is exactly zero in both.
    measured: x_1, x_2, x_3, x_6 3.7e-6 at worst (D = 252, e32 1.9e-6; 4.0 .. 4.8 x e32 at n_proto = 90 and n = 257, the same
    at every T: the error of S in the top mode, in x_0 already -- profiles/r33_cg_coarse.md); r_1 1.30e-5 (e32 5.4e-6),
    r_2 1.26e-5 (1.9e-5), r_3 2.06e-5 (3.3e-5); r_6 8.05e-4 (7.1e-4) on 31 nodes around 12 prototypes, a case since
    replaced (fp32 cannot hold that residual; the cases' own fp32 figures are asserted on the host), below 5e-5 elsewhere."""
    c, f = sol.case, sol.ref
    assert min(f.count(f.run, 1e-6), f.count(f.run32, 1e-6)) > max(EARLY)
    errs, e32 = {}, {}
    for T in EARLY:
        run = sol.runs["lds", "T", T]
        _finite(run, c.n)
        assert run["stats"].tolist() == [0, T], "%s T=%d: stats %s" % (c.name, T, run["stats"].tolist())
        assert (run["Z"][:, 3] == 0).all() and (run["r"][:, 3] == 0).all(), "the all-zero column did not stay zero"
        assert (run["r"][c.n:] == 0).all()
        errs["x%d" % T] = C.rel(run["Z"], f.run.xs[T])
        errs["r%d" % T] = C.rel(run["r"][:c.n], f.run.rs[T])
        e32["x%d" % T] = C.rel(f.run32.xs[T], f.run.xs[T])
        e32["r%d" % T] = C.rel(f.run32.rs[T], f.run.rs[T])
    _hold(c.name, errs, e32)


# ----------------------------------------------------------------------------------------------------------------------
# e. iteration count
# ----------------------------------------------------------------------------------------------------------------------
def _count(c, f, i, tol, conv, iters):
    k64, k32, plain = f.count(f.run, tol), f.count(f.run32, tol), f.count(f.plain, tol)
    windowed, unstable = (c.name, tol) in CC.COUNT_WINDOW, (c.name, tol) in CC.UNSTABLE
    spread = sorted({p[i] for p in C.perturbed_counts(c, f)}) if unstable else []
    print("CGC| %-8s tol %g: iterations device %d / float64 %d / fp32 %d / plain %d%s" % (
        c.name, tol, iters, k64, k32, plain,
        "" if windowed else "  (fp32 under one-ulp perturbations of S: %s)" % spread if unstable else "  (no window: near the threshold)"))
    assert conv == 1, (c.name, tol, conv, iters)
    if windowed:
        assert f.run.ratio(k64, tol) < 0.5 and f.run.ratio(k64 - 1, tol) > 2.0
        assert min(k64, k32) - 1 <= iters <= max(k64, k32) + 1, (c.name, tol, iters, k64, k32)
    if unstable:  # (the spread printed above is this host's and asserts nothing: another host's BLAS draws another)
        assert k64 - 1 <= iters <= k64 + CC.UNSTABLE_SPREAD + 1, (c.name, tol, iters, k64, k32, spread)
    else:
        assert iters <= plain, (c.name, tol, iters, plain)


def test_e_iteration_count(sol):
    """tol 1e-6 and 1e-7, max_iter 300: converged == 1; iters within [min, max] of the float64 and the fp32 host runs of
    the restatement, widened by one on each side, for the (case, tol) pairs of cg_cases.COUNT_WINDOW -- those whose float64
    residual passes the test by a factor 2 at its stopping iteration and misses it by 2 one earlier (asserted here) and
    whose fp32 count one-ulp perturbations of S do not move (asserted in tests/test_cg_ref_host.py); and never more than
    plain float64 CG needs.  The two pairs of cg_cases.UNSTABLE (one and two aggregates at 1e-7, where the fp32
    restatement itself counts 17 or 21 depending on the last bit of S) are held to float64's count - 1 .. + 5: the spread
    of the perturbed restatements recorded in profiles/r33_cg_coarse.md (0 or 4 late, both cases), widened by one.
    measured: the device's count EQUALS the float64 and the fp32 host count in every windowed pair (8 .. 21 iterations,
    plain CG 10 .. 50); proto1 at 1e-7: 21 (float64 17, perturbed fp32 17 and 21); profiles/r33_cg_coarse.md has the table."""
    c, f = sol.case, sol.ref
    for i, tol in enumerate(CC.TOLS):
        run = sol.runs["lds", "tol", tol]
        _finite(run, c.n)
        conv, iters = run["stats"].tolist()
        _count(c, f, i, tol, conv, iters)
        assert (run["Z"][:, 3] == 0).all()
    # the converged Z beside the early iterates' figures: what the SYSTEM's fp32 rounding (S, amplified by up to
    # 1 / (1 - alpha) in the top mode) puts into every iterate from x_0 on, whatever the preconditioner does
    _hold(c.name, dict(Z=C.rel(sol.runs["lds", "tol", 1e-7]["Z"], f.run.xs[-1])), dict(Z=C.rel(f.run32.xs[-1], f.run.xs[-1])))


# ----------------------------------------------------------------------------------------------------------------------
# f. batch
# ----------------------------------------------------------------------------------------------------------------------
def test_f_batch_of_two(ops):
    """E = 2 systems of different n and n_proto in one capacity: each against its own float64 reference (aggregates exact,
    stats, MW / Einv / early iterates at the module's bars), and each bit for bit its E = 1 call in the same capacity --
    agg, MW, Einv, Z, r and stats -- with the whole lp_ws full of NaN and NaN node rows beyond n before every call, under
    both SpMV forms."""
    cases = [CC.get(nm) for nm in CC.BATCH]
    nc = max(c.n for c in cases) + CC.CAP_EXTRA
    hb2 = _buffers(ops, nc, cases[0].D, 2)
    nbr2 = _load(ops, hb2, cases)
    both = _runs(ops, hb2, nbr2, cases)
    for e, c in enumerate(cases):
        _check_csr(hb2, e, c)
        hb1 = _buffers(ops, nc, c.D, 1)
        nbr1 = _load(ops, hb1, [c])
        one = _runs(ops, hb1, nbr1, [c])
        f = C.reference(c)
        for key in both:
            _same_bits(both[key][e], one[key][0], "%s %s: E = 2 against E = 1" % (c.name, key))
            _same_bits(both[key][e], both[("lds",) + key[1:]][e], "%s %s: form against form" % (c.name, key))
            assert torch.equal(both[key][e]["agg"], f.agg)
        run = both["lds", "T", 1][e]
        co = C.coarse(f.S, f.dinv, run["agg"], c.alpha)
        keep = torch.nonzero(~co.empty).squeeze(1)
        I = torch.eye(len(keep), dtype=torch.float64)
        errs = dict(MW=C.rel(run["MW"][:c.n], co.MW),
                    Einv=(run["Einv"][keep][:, keep].double() @ co.E[keep][:, keep] - I).abs().max().item())
        e32 = dict(MW=C.rel(f.co32.MW, f.co.MW),
                   Einv=(f.co32.Einv[keep][:, keep].double() @ f.co.E[keep][:, keep] - I).abs().max().item())
        assert (run["MW"][c.n:] == 0).all()
        for T in EARLY:
            rT = both["lds", "T", T][e]
            assert rT["stats"].tolist() == [0, T]
            errs["x%d" % T], e32["x%d" % T] = C.rel(rT["Z"], f.run.xs[T]), C.rel(f.run32.xs[T], f.run.xs[T])
            errs["r%d" % T], e32["r%d" % T] = C.rel(rT["r"][:c.n], f.run.rs[T]), C.rel(f.run32.rs[T], f.run.rs[T])
        _hold("E2:" + c.name[:5], errs, e32)
        for i, tol in enumerate(CC.TOLS):
            assert (c.name, tol) in CC.COUNT_WINDOW
            _count(c, f, i, tol, *both["lds", "tol", tol][e]["stats"].tolist())
