"""Dense restatement of the two-level conjugate gradients of csrc/head_graph.hip, section 5 (the A-DEF2 preconditioner),
in plain torch on the CPU, for tests/test_gpu_cg_coarse.py; tests/test_cg_ref_host.py holds it to its own algebra and to
head_ref.lp_dense's closed form without a GPU.

Every function takes a ``dtype``: float64 is the reference, float32 the same formulas in the kernels' precision (the
``e32`` the GPU tests print beside each measured figure, and the second iteration count of a case).  Nothing here is
fitted to what the device gives: the definitions are those of the comment block of section 5,

    seeds       src[s] = floor(s (n_proto - 1) / 63), s = 0 .. 63, n_proto clamped to [1, n]
    aggregate   agg[i] = arg-min_s || x_i - x_src[s] ||^2, ties to the lower seed
    u = D^1/2 = 1 / dinv,  W = diag(u) [agg == a],  M = I - alpha S,  MW = M W
    E = (W^T M W + (W^T M W)^T) / 2, an EMPTY aggregate's zero row and column given a unit diagonal;  Einv = E^-1
    x_0 = W Einv W^T b,  r_0 = b - MW Einv W^T b
    z = r + W mu,  mu = Einv (W^T r - (MW)^T r);  <r, z> = <r, r> + <W^T r, mu>
    p = z + beta p,  q = M r + MW mu + beta q  (= M p, by recurrence as the kernels form it)
    a = <r, z> / <p, q>,  x += a p,  r -= a q,  beta = <r, z>_new / <r, z>_old

with one a and one beta PER COLUMN of the right-hand side (the columns are independent systems that share the matrix).
A coefficient whose denominator is not positive is zero (the kernels' guards: a column that is all zero stays zero).
"""
import numpy as np
import torch

import head_ref as R

HG_M = 64   # aggregates = coarse dimensions


# ----------------------------------------------------------------------------------------------------------------------
# the graph: head_ref.lp_from_nodes' formulas, with the degree vector kept (the coarse space needs D^1/2)
# ----------------------------------------------------------------------------------------------------------------------
def graph(x, nbr, sigma, dtype=torch.float64):
    """x (n, D), nbr (n, k + 1) int64 (column 0 dropped) -> (S (n, n), dinv (n,)) in `dtype`: the affinity of
    head_ref.lp_from_nodes, line by line, returned with dinv = sqrt(1 / (rowsum + eps))."""
    xl = x.detach().to(dtype)
    n, d = xl.shape
    I = nbr[:, 1:]
    k = I.shape[1]
    knn_feat = xl[I.reshape(-1)].view(n, k, d)
    dist = torch.norm(xl[:, None, :] - knn_feat + 1e-6, 2, 2)
    w = torch.exp(-0.5 * (dist / sigma) ** 2)
    A = torch.zeros(n, n, dtype=dtype).scatter(1, I, w)
    A = A + A.t()
    A = A * (1 - torch.eye(n, dtype=dtype))
    dinv = torch.sqrt(1.0 / (A.sum(1) + R.EPS))
    return dinv[:, None] * A * dinv[None, :], dinv


def pattern(nbr):
    """(n, n) bool: the symmetrised pattern of the lists (column 0 dropped, diagonal dropped) -- what the CSR must hold."""
    n = nbr.shape[0]
    adj = torch.zeros(n, n, dtype=torch.bool)
    adj[torch.arange(n)[:, None].expand(-1, nbr.shape[1] - 1), nbr[:, 1:]] = True
    adj |= adj.t().clone()
    adj[torch.arange(n), torch.arange(n)] = False
    return adj


# ----------------------------------------------------------------------------------------------------------------------
# 5a. seeds and aggregates
# ----------------------------------------------------------------------------------------------------------------------
def seeds(n_proto, n):
    """Node row of each of the 64 seeds: floor(s (n_proto - 1) / 63), n_proto clamped to [1, n] -> (64,) int64."""
    n_proto = max(1, min(int(n_proto), int(n)))
    return torch.tensor([(s * (n_proto - 1)) // (HG_M - 1) for s in range(HG_M)], dtype=torch.int64)


def aggregates(x, src, dtype=torch.float64):
    """x (n, D), src (64,) -> (agg (n,) int64, gap (n,) float64).  agg: arg-min over the seeds of the squared L2 distance to
    the seed ROW x[src[s]] (differences first, then squares), ties -- duplicated seed rows -- to the lower seed.  gap: per
    node (second - best) / second over the DISTINCT distance values, inf where every seed is at the same distance (one
    distinct seed row): how far the decision is from a tie that rounding could turn."""
    xd = x.detach().to(dtype)
    d2 = ((xd[:, None, :] - xd[src][None, :, :]) ** 2).sum(2).numpy()        # (n, 64)
    agg = d2.argmin(1)                                                      # numpy: the FIRST minimum
    best = d2.min(1)
    rest = np.where(d2 > best[:, None], d2, np.inf)
    second = rest.min(1)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(second), (second - best) / np.where(np.isfinite(second), second, 1.0), np.inf)
    return torch.from_numpy(agg.astype(np.int64)), torch.from_numpy(gap.astype(np.float64))


# ----------------------------------------------------------------------------------------------------------------------
# 5b, 5c. the coarse space of a given partition
# ----------------------------------------------------------------------------------------------------------------------
class Coarse:
    """u, W (n, 64), M (n, n), MW (n, 64), E (64, 64), Einv (64, 64), empty (64,) bool -- all in one dtype."""


def coarse(S, dinv, agg, alpha, dtype=torch.float64):
    S, dinv = S.to(dtype), dinv.to(dtype)
    n = S.shape[0]
    c = Coarse()
    c.u = 1.0 / dinv
    c.W = torch.zeros(n, HG_M, dtype=dtype)
    c.W[torch.arange(n), agg] = c.u
    c.M = torch.eye(n, dtype=dtype) - alpha * S
    c.MW = c.M @ c.W
    E0 = c.W.t() @ c.MW
    c.E = 0.5 * (E0 + E0.t())
    c.empty = torch.bincount(agg, minlength=HG_M) == 0
    idx = torch.nonzero(c.empty).squeeze(1)
    c.E[idx, idx] = 1.0                     # (row and column of an empty aggregate are exactly zero: W's column is)
    c.Einv = torch.linalg.inv(c.E)
    return c


# ----------------------------------------------------------------------------------------------------------------------
# the iteration
# ----------------------------------------------------------------------------------------------------------------------
def _safe_div(a, b):
    return torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), torch.zeros_like(a))


class Run:
    """xs [x_0 .. x_iters], rs [r_0 .. r_iters] (the recurrence's residuals), rho [k] = (rr_k, bb) per column,
    converged, iters."""

    def ratio(self, k, tol):
        """max over the columns of rr_k / (tol^2 bb); a column with bb == 0 counts 0 when rr_k == 0, else inf."""
        rr, bb = self.rr[k], self.bb
        t = torch.where(bb > 0, rr / (tol * tol * torch.where(bb > 0, bb, torch.ones_like(bb))),
                        torch.where(rr > 0, torch.full_like(rr, float("inf")), torch.zeros_like(rr)))
        return t.max().item()

    def stop(self, tol):
        """The first k whose residual passes the test at `tol` (None: none of the recorded ones does)."""
        for k in range(len(self.rr)):
            if bool((self.rr[k] <= tol * tol * self.bb).all()):
                return k
        return None


def two_level_cg(c, Y, max_iter, tol, dtype=torch.float64, two_level=True):
    """CG on M X = Y with the coarse space c (two_level=False: plain CG, x_0 = 0, z = r), every quantity in `dtype`.

    THE COUNT'S CONVENTION, read from the kernels: r3d_cg_init_kernel (mode 1) forms x_0, r_0 and its last workgroup runs
    cg_reduce_step(phase 1, it = 0); every r3d_cg_update_kernel(it) -- or the head of the fused launch it + 1 -- forms
    x_{it+1}, r_{it+1} and runs cg_reduce_step(phase 1, it + 1).  The step FIRST tests rr_k <= tol^2 bb for all four
    columns (rr_k = <r_k, r_k>, bb = <b, b>, both as stored, `<=`): if it holds it sets done = 1, iters = k and leaves;
    else it stores iters = k with the coefficients of iteration k.  Launches after `done` return at once, and the host
    issues max_iter updates.  So CgState::iters is the NUMBER OF UPDATES APPLIED = the index k of the iterate x_k that
    Z holds: the smallest k in 0 .. max_iter whose residual passes the test (converged = 1; k = 0: x_0 already passes,
    e.g. b = 0), or max_iter with converged = 0 when none does -- the test after the last update counts, so a system
    whose x_{max_iter} passes IS converged.  r3d_cg_stats_kernel copies {done, iters} (done as 0 after a given-up wait)."""
    M, W, MW, Einv = c.M.to(dtype), c.W.to(dtype), c.MW.to(dtype), c.Einv.to(dtype)
    b = Y.to(dtype)
    n, C = b.shape
    run = Run()
    run.bb = (b * b).sum(0)
    if two_level:
        c0 = Einv @ (W.t() @ b)
        x = W @ c0
        r = b - MW @ c0
    else:
        x = torch.zeros_like(b)
        r = b.clone()
    p, q = torch.zeros_like(b), torch.zeros_like(b)
    rz_old = torch.zeros(C, dtype=dtype)
    run.xs, run.rs, run.rr = [x.clone()], [r.clone()], []
    run.converged, run.iters = 0, max_iter
    for k in range(max_iter + 1):
        rr = (r * r).sum(0)
        run.rr.append(rr)
        if bool((rr <= tol * tol * run.bb).all()):
            run.converged, run.iters = 1, k
            break
        if k == max_iter:
            break
        if two_level:
            t = W.t() @ r
            mu = Einv @ (t - MW.t() @ r)
            rz = rr + (t * mu).sum(0)
        else:
            mu = torch.zeros(HG_M, C, dtype=dtype)
            rz = rr
        beta = _safe_div(rz, rz_old) if k > 0 else torch.zeros(C, dtype=dtype)
        rz_old = rz
        p = (r + W @ mu) + beta * p
        q = (M @ r + MW @ mu) + beta * q
        a = _safe_div(rz, (p * q).sum(0))
        x = x + a * p
        r = r - a * q
        run.xs.append(x.clone())
        run.rs.append(r.clone())
    return run


def problem(case, dtype=torch.float64):
    """Everything of a tests/cg_cases.py case in one precision: S, dinv, seeds, aggregates + gaps."""
    S, dinv = graph(case.x, case.nbr, case.sigma, dtype)
    src = seeds(case.n_proto, case.n)
    agg, gap = aggregates(case.x, src, dtype)
    return S, dinv, src, agg, gap


REF_TOL, REF_ITERS = 1e-7, 300   # the reference runs stop at the tighter tolerance: the count at 1e-6 is Run.stop(1e-6)
_refs = {}


class Ref:
    """Of one case, computed once and left unchanged: S, dinv, src, agg, gap, co (float64 coarse space of agg), co32 (the
    same restatement in fp32 on the SAME partition), run / run32 (two-level, float64 / fp32), plain (plain CG, float64)."""

    def count(self, run, tol):
        k = run.stop(tol)
        assert k is not None, "the reference run did not reach tol %g" % tol
        return k


def perturbed_counts(case, f, n_pert=8):
    """How firmly fp32 decides the count: the fp32 restatement on S (1 + P), P symmetric with entries ~ 6e-8 N(0, 1) (about
    one ulp), n_pert times -> [(count at 1e-6, count at 1e-7)].  Computed once per case."""
    if not hasattr(f, "_pert"):
        g = torch.Generator().manual_seed(1)
        S32, dinv32 = graph(case.x, case.nbr, case.sigma, torch.float32)
        f._pert = []
        for _ in range(n_pert):
            P = torch.randn(S32.shape, generator=g) * 6e-8
            co = coarse(S32 * (1 + (P + P.t()) / 2), dinv32, f.agg, case.alpha, torch.float32)
            run = two_level_cg(co, case.Y, REF_ITERS, REF_TOL, torch.float32)
            f._pert.append((run.stop(1e-6), run.stop(1e-7)))
    return f._pert


def reference(case):
    if case.name not in _refs:
        with torch.no_grad():
            f = Ref()
            f.S, f.dinv, f.src, f.agg, f.gap = problem(case)
            f.co = coarse(f.S, f.dinv, f.agg, case.alpha)
            S32, dinv32 = graph(case.x, case.nbr, case.sigma, torch.float32)
            f.co32 = coarse(S32, dinv32, f.agg, case.alpha, torch.float32)
            f.run = two_level_cg(f.co, case.Y, REF_ITERS, REF_TOL)
            f.run32 = two_level_cg(f.co32, case.Y, REF_ITERS, REF_TOL, torch.float32)
            f.plain = two_level_cg(f.co, case.Y, 500, REF_TOL, two_level=False)
        _refs[case.name] = f
    return _refs[case.name]


rel = R.rel
