"""The head's training backward, kernel by kernel, against float64 at every feature width: r3d_ce_grad_batched,
r3d_label_propagate(_solve)_batched / _bwd_batched, r3d_head_prototypes(_bwd)_batched, r3d_contrast_fwd / _bwd
(csrc/head_graph.hip, head_proto.hip, contrast.hip) through the C ABI.

References: tests/head_ref.py (the reference's formulas in float64; held to the fp32 oracle in tests/test_head_ref_host.py).
Index decisions -- neighbour lists, FPS seeds, assignments -- are the oracle's on the fp32 inputs, the neighbour lists
checked equal to the device's first.

Bars.  Every figure is max |got - ref64| / max |ref64| over the named block.  Each test prints it beside ``e32``, the error
the SAME dense formula makes in fp32 on the CPU against float64 on that input.  A bar is 4 x the worst error measured on the
MI355X for that quantity over this module's cases (the kernels are deterministic: the margin covers other seeds) and never
above CEIL = 1e-3.  The measured figures stand in each test's docstring."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import head_ref as R
from proto_cases import masks as _masks  # exact foreground counts per (way, shot)
from oracle import r3d_oracle as O

pytestmark = pytest.mark.gpu

CEIL = 1e-3
# quantity -> bar = 4 x the worst figure measured over the module's cases (the figures: each test's docstring)
BAR = dict(S=1.2e-6,            # 3.00e-7 (A, D = 192 k = 200)
           Z=8.3e-6,            # 2.07e-6 (A, D = 192 k = 200)
           lam=9.9e-6,          # 2.47e-6 (A, D = 256 k = 8)
           dnodes=2.9e-5,       # 7.34e-6 (B, system 1, query rows, channels [64, 128))
           G=3.8e-7,            # 9.59e-8 (D, 2 classes)
           nodes=1.8e-7,        # 4.59e-8 (E, D = 64)
           dsfeat=8.5e-8,       # 2.12e-8 (E, D = 256)
           dqfeat=0.0,          # a copy
           closs=4.2e-7,        # 1.05e-7 (F, D = 64)
           cdfeat=1.2e-5,       # 2.88e-6 (F, D = 256, noisy)
           cdW=9.4e-6,          # 2.35e-6 (F, D = 256, noisy)
           cdb=9.0e-6,          # 2.26e-6 (F, D = 256, noisy)
           chain_loss=5.2e-6,   # 1.29e-6 (G)
           chain_dfeat=3.6e-5)  # 8.88e-6 (G)
assert max(BAR.values()) <= CEIL


@pytest.fixture(scope="module")
def ops():
    from r3dfsseg_amd import ops as _ops
    from r3dfsseg_amd import _lib
    _lib.load()
    return _ops


def _report(case, errs, e32):
    for k in errs:
        print("HB| %-34s %-18s err %.2e  e32 %.2e" % (case, k, errs[k], e32.get(k, float("nan"))))


def _hold(case, errs, e32, bars):
    """Print every figure, then assert every one (bars: quantity -> bar; a key 'dnodes:proto[0:64)' takes the bar of
    'dnodes')."""
    _report(case, errs, e32)
    bad = {k: v for k, v in errs.items() if not v <= bars[k.split(":")[0]]}
    assert not bad, (case, bad)


# ----------------------------------------------------------------------------------------------------------------------
# A - C: graph, solve and adjoint
# ----------------------------------------------------------------------------------------------------------------------
TABLE_A = [(256, 8, 70, 530, 1.0), (132, 40, 70, 530, 1.0), (192, 200, 90, 530, 1.0), (64, 16, 40, 300, 0.5),
           (224, 200, 90, 530, 1.0)]
ALPHA, TOL, ITERS = 0.99, 1e-7, 300
_ref_cache = {}


def _system(D, n_proto, n_q_pts, planes, seed=1):
    """-> (x (n, D), Y (n, 4 planes): one-hot on the prototype rows, zero on the query rows)."""
    x, lab = R.graph_nodes(n_proto, n_q_pts, D, seed)
    n = n_proto + n_q_pts
    g = torch.Generator().manual_seed(1000 + seed)
    Y = torch.zeros(n, 4 * planes)
    cls = lab[:n_proto] if planes == 1 else torch.randint(0, 8, (n_proto,), generator=g)
    Y[torch.arange(n_proto), cls] = 1
    return x, Y


def _lp_reference(key, x, nbr, Y, G, sigma):
    """float64 (and fp32, for e32) dense reference of one system, computed once per case and shared."""
    if key not in _ref_cache:
        r64 = R.lp_dense_grad(x, nbr, Y, G, sigma, ALPHA)
        r32 = R.lp_dense_grad(x, nbr, Y, G, sigma, ALPHA, dtype=torch.float32)
        _ref_cache[key] = (r64, r32)
    return _ref_cache[key]


def _run_lp(ops, systems, D, k_connect, sigma, planes=1, cap=None, again=None):
    """Forward + adjoint of len(systems) systems (n_proto, n_q_pts) in ONE call each, inside the capacity of `cap` (default:
    the first system) plus spare prototype slots: n < n_cap for every system.  Rows n .. n_cap of the node matrix hold
    7.0, of dnodes a poison, of G random numbers.  again: results of an earlier call whose nodes, Y and rows < n of G
    are used again (with other numbers beyond n).  -> per system a dict of host tensors."""
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    E = len(systems)
    n_way = 2 if planes == 1 else 4
    cp, cq = cap or systems[0]
    k_sub = cp // (n_way + 1) + 2
    hb = ops.HeadBuffers(n_way, 1, cq, cq, k_sub, k_connect, D, "cuda", E=E)
    assert hb.planes == planes and all(hb.n_cap > p + q for p, q in systems)
    nc, pl = hb.n_cap, E * hb.n_cap
    desc = hb.desc.view(E, 32)
    hb.nodes.fill_(7.0)  # garbage beyond n must be ignored
    hb.Y.zero_()
    inputs = []
    gG = torch.Generator().manual_seed(77 if again is None else 78)
    G = torch.randn(planes, E, nc, 4, generator=gG)  # random on all four columns of every row, prototype rows included
    for e, (n_proto, n_q_pts) in enumerate(systems):
        x, Y = _system(D, n_proto, n_q_pts, planes, seed=1 + e) if again is None else (again[e]["x"], again[e]["Y"])
        n = n_proto + n_q_pts
        if again is not None:
            G[:, e, :n] = again[e]["G"].view(n, planes, 4).transpose(0, 1)
        hb.nodes[e * nc:e * nc + n] = x.cuda()
        for p in range(planes):
            hb.Y[p * pl + e * nc:p * pl + e * nc + n] = Y[:, 4 * p:4 * p + 4].cuda()
        desc[e, ops.HD_N_PROTO] = n_proto
        desc[e, ops.HD_N_NODES] = n
        inputs.append((x, Y, n))
    nbr = ops.knn_nodes(hb)
    assert int(hb.knn_status.item()) == 0
    Z = ops.label_propagate(hb, nbr, sigma, ALPHA, ITERS, TOL)
    Gd = G.reshape(planes * pl, 4).cuda()
    lam = torch.empty(planes * pl, 4, device="cuda")
    dnodes = torch.full((planes, pl, D), float("nan"), device="cuda")  # (rows >= n stay poisoned: never read back)
    stats_b = torch.zeros(planes, E, 2, device="cuda", dtype=torch.int32)
    for p in range(planes):  # once per plane, the results add (head_train.lp_backward)
        _lib.check(lib.r3d_label_propagate_bwd_batched(
            E, ops._p(hb.nodes), hb.nodes.stride(0), D, hb.kp1, ops._p(Z[p * pl:]), ops._p(Gd[p * pl:]),
            ops._p(hb.n_nodes_ptr()), 32, nc, float(sigma), ALPHA, ITERS, TOL, ops._p(lam[p * pl:]), ops._p(dnodes[p]), D,
            ops._p(hb.lp_ws), hb.lp_words, hb.lp_stride, ops._p(stats_b[p]), 2, ops._st()))
    torch.cuda.synchronize()
    stats_f = hb.stats.view(E, 2).cpu()
    nbr_h = nbr.view(E, nc, hb.kp1).cpu().to(torch.int64)
    Zh, lamh = Z.view(planes, E, nc, 4).cpu(), lam.view(planes, E, nc, 4).cpu()
    dn = dnodes.view(planes, E, nc, D).cpu()
    out = []
    for e, (x, Y, n) in enumerate(inputs):
        _, row_ptr, col, val = hb.csr(e)
        out.append(dict(x=x, Y=Y, n=n, n_proto=systems[e][0], nbr=nbr_h[e, :n], G=torch.cat(list(G[:, e, :n]), 1),
                        Z=torch.cat(list(Zh[:, e, :n]), 1), lam=torch.cat(list(lamh[:, e, :n]), 1),
                        dnodes=dn[:, e, :n].sum(0), dn_tail=dn[:, e, n:], row_ptr=row_ptr.cpu(), col=col.cpu(), val=val.cpu(),
                        conv_f=int(stats_f[e, 0]), conv_b=stats_b[:, e, 0].cpu().tolist(), iters_f=int(stats_f[e, 1]),
                        iters_b=stats_b[:, e, 1].cpu().tolist()))
    return out


def _check_system(case, key, r, sigma):
    """One system of _run_lp against its float64 reference: assertions 1-7 of the graph-and-adjoint case."""
    x, Y, n, n_proto = r["x"], r["Y"], r["n"], r["n_proto"]
    want_nbr = O.knn_l2(x, r["nbr"].shape[1])
    assert torch.equal(r["nbr"], want_nbr), "%s: neighbour lists differ from the oracle's" % case
    assert (r["nbr"][n_proto + 9, :2] == torch.tensor([n_proto + 8, n_proto + 9])).all()  # own index at column 1
    assert r["conv_f"] == 1, "%s: CG did not converge (%d iterations)" % (case, r["iters_f"])
    assert all(c == 1 for c in r["conv_b"]), "%s: the adjoint CG did not converge %s" % (case, r["iters_b"])  # 7
    (S, Z, lam, dx), (S32, Z32, lam32, dx32) = _lp_reference(key, x, r["nbr"], Y, r["G"], sigma)
    # 1. exactly the non-zero pattern of S
    rows = torch.repeat_interleave(torch.arange(n), r["row_ptr"][1:] - r["row_ptr"][:-1])
    assert r["row_ptr"][0] == 0 and len(rows) == len(r["col"]) and int(r["col"].max()) < n
    Sd = torch.zeros(n, n, dtype=torch.float64)
    pat = torch.zeros(n, n, dtype=torch.bool)
    pat[rows, r["col"]] = True
    assert int(pat.sum()) == len(rows), "%s: a CSR row lists a column twice" % case
    assert torch.equal(pat, S != 0), "%s: the CSR pattern is not the pattern of S" % case
    assert not torch.diagonal(pat).any()
    Sd[rows, r["col"]] = r["val"].double()
    rowlen = pat.sum(1)
    assert torch.isfinite(r["dnodes"]).all() and torch.isnan(r["dn_tail"]).all()  # 6: rows >= n are not written
    errs = dict(S=R.rel(Sd, S), Z=R.rel(r["Z"], Z), lam=R.rel(r["lam"], lam))
    e32 = dict(S=R.rel(S32, S), Z=R.rel(Z32, Z), lam=R.rel(lam32, lam))
    for k, v in R.block_errors(r["dnodes"], dx, n_proto).items():
        errs["dnodes:" + k] = v
    for k, v in R.block_errors(dx32, dx, n_proto).items():
        e32["dnodes:" + k] = v
    print("HB| %-34s rows %d..%d long, CG %d / adjoint %s iterations" % (case, int(rowlen.min()), int(rowlen.max()),
                                                                        r["iters_f"], r["iters_b"]))
    _hold(case, errs, e32, BAR)
    return int(rowlen.max())


@pytest.mark.parametrize("D,k_connect,n_proto,n_q_pts,sigma", TABLE_A)
def test_graph_and_adjoint(ops, D, k_connect, n_proto, n_q_pts, sigma):
    """A.  CSR pattern and values of S, Z, lam = inv(I - alpha S) G and dnodes = d<Z, G>/dx for a random G, per block of
    rows (prototype / query) and channels, at widths that take every path of r3d_graph_weights_kernel (six-float4 trip,
    remainder loop) and r3d_lp_bwd_dx_kernel (channel clamp, fourth group, rows longer than one 256-entry chunk), with
    a hub row, duplicated nodes (a self-edge at column 1), n < n_cap and poisoned rows beyond n.
    measured, worst over the blocks (e32 in brackets):
      D 256 k   8: S 1.5e-7 (2.4e-7)  Z 1.8e-6 (8.9e-7)  lam 2.5e-6 (1.1e-6)  dnodes 2.0e-6 (1.5e-6)  rows 8..71
      D 132 k  40: S 2.0e-7 (2.1e-7)  Z 1.0e-6 (1.5e-6)  lam 1.2e-6 (1.7e-6)  dnodes 3.4e-6 (4.6e-6)  rows 40..169
      D 192 k 200: S 3.0e-7 (2.9e-7)  Z 2.1e-6 (2.3e-6)  lam 1.4e-6 (2.9e-6)  dnodes 2.7e-6 (4.2e-6)  rows 200..397
      D  64 k  16: S 2.1e-7 (2.0e-7)  Z 1.2e-6 (1.3e-6)  lam 1.6e-6 (1.2e-6)  dnodes 2.2e-6 (8.5e-6)  rows 16..84
      D 224 k 200: S 2.7e-7 (2.9e-7)  Z 1.9e-6 (2.0e-6)  lam 2.3e-6 (2.7e-6)  dnodes 2.5e-6 (2.9e-6)  rows 200..401
    12 - 13 CG iterations forward and adjoint."""
    r = _run_lp(ops, [(n_proto, n_q_pts)], D, k_connect, sigma)[0]
    longest = _check_system("A D=%d k=%d" % (D, k_connect), ("A", D, k_connect, n_proto, n_q_pts), r, sigma)
    if k_connect == 200:
        assert longest > 256  # the hub: more than one chunk of the dx kernel's walk


def test_two_systems_of_different_size_in_one_call(ops):
    """B.  E = 2: system 0 = the first row of the table, system 1 shorter (n_proto 50, 400 query points) inside the same
    capacity.  Each holds its own float64 reference and equals the E = 1 call on it bit for bit.
    measured (system 1; system 0 is case A's): S 1.8e-7 (e32 1.7e-7)  Z 2.1e-6 (2.2e-6)  lam 1.7e-6 (2.3e-6)
    dnodes 7.3e-6 (4.5e-6), rows 8..91."""
    D, k_connect, n_proto, n_q_pts, sigma = TABLE_A[0]
    systems = [(n_proto, n_q_pts), (50, 400)]
    both = _run_lp(ops, systems, D, k_connect, sigma)
    _check_system("B sys 0 of 2", ("A", D, k_connect, n_proto, n_q_pts), both[0], sigma)
    _check_system("B sys 1 of 2", ("B1", D, k_connect), both[1], sigma)
    for e in (0, 1):
        alone = _run_lp(ops, [systems[e]], D, k_connect, sigma, cap=systems[0], again=[both[e]])[0]
        for k in ("Z", "lam", "dnodes", "val", "col", "row_ptr"):
            assert torch.equal(both[e][k], alone[k]), "system %d of the batch differs from the E = 1 call in %s" % (e, k)


def test_two_planes(ops):
    """C.  Eight label columns as two planes of four: plane 0 solved by r3d_label_propagate_batched, plane 1 by
    r3d_label_propagate_solve_batched on the same graph, the adjoint once per plane and the planes' dnodes added;
    against float64 with 8 label columns, D = 256 (the fourth channel group), k_connect = 8.
    measured: S 1.5e-7 (e32 2.4e-7)  Z 1.8e-6 (9.5e-7)  lam 2.5e-6 (1.1e-6)  dnodes 3.0e-6 (1.8e-6)."""
    D, k_connect, n_proto, n_q_pts, sigma = TABLE_A[0]
    r = _run_lp(ops, [(n_proto, n_q_pts)], D, k_connect, sigma, planes=2)[0]
    assert r["Y"][:, 4:].sum() > 0 and r["Z"].shape[1] == 8
    _check_system("C two planes", ("C", D, k_connect), r, sigma)


def test_the_adjoint_refuses_a_width_that_is_no_multiple_of_4(ops):
    """D = 130 with ldn = 132: the forward refuses it (its coarse space stages the seed rows as whole float4 and would
    leave channels 128, 129 of the seeds unset); the backward, which runs on the forward's workspace, refuses it alike --
    an error code before any launch, nothing written."""
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    hb = ops.HeadBuffers(2, 1, 64, 64, 4, 8, 132, "cuda")
    hb.nodes.zero_(); hb.Y.zero_(); hb.Z.zero_()
    hb.desc[0, ops.HD_N_PROTO] = 10
    hb.desc[0, ops.HD_N_NODES] = 74
    nbr = torch.zeros(hb.n_cap, hb.kp1, device="cuda", dtype=torch.int32)
    G = torch.zeros(hb.n_cap, 4, device="cuda")
    lam = torch.full((hb.n_cap, 4), 3.0, device="cuda")
    dn = torch.full((hb.n_cap, 132), 3.0, device="cuda")
    fwd = lambda D: lib.r3d_label_propagate_batched(
        1, ops._p(hb.nodes), 132, D, ops._p(nbr), hb.kp1, ops._p(hb.Y), ops._p(hb.n_nodes_ptr()), ops._p(hb.n_proto_ptr()), 32,
        hb.n_cap, 1.0, ALPHA, 8, TOL, ops._p(hb.Z), ops._p(hb.lp_ws), hb.lp_words, hb.lp_stride, ops._p(hb.stats), 2, ops._st())
    bwd = lambda D: lib.r3d_label_propagate_bwd_batched(
        1, ops._p(hb.nodes), 132, D, hb.kp1, ops._p(hb.Z), ops._p(G), ops._p(hb.n_nodes_ptr()), 32, hb.n_cap, 1.0, ALPHA, 8, TOL,
        ops._p(lam), ops._p(dn), 132, ops._p(hb.lp_ws), hb.lp_words, hb.lp_stride, ops._p(hb.stats_bwd), 2, ops._st())
    for D in (130, 131, 129):
        assert fwd(D) != 0 and "D=%d" % D in lib.r3d_last_error_string().decode()
        assert bwd(D) != 0 and "D=%d" % D in lib.r3d_last_error_string().decode()
    torch.cuda.synchronize()
    assert (lam == 3.0).all() and (dn == 3.0).all() and (hb.Z == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# D: gradient of the cross entropy
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_classes", [2, 3, 4, 5, 8])
def test_ce_grad(ops, n_classes):
    """D.  r3d_ce_grad_batched, E = 2 with different n_proto, gscale 0.37, Z random at scale 3; more than 4 classes: two
    planes.  Rows outside [n_proto, n_proto + n_qpts) and columns >= n_classes exactly zero.
    measured: G 9.6e-8 at worst (e32 1.0e-7)."""
    E, n_cap, n_qpts, gscale = 2, 300, 200, 0.37
    planes = 1 if n_classes <= 4 else 2
    n_proto = [37, 61]
    g = torch.Generator().manual_seed(n_classes)
    Z = torch.randn(planes, E, n_cap, 4, generator=g) * 3
    labels = torch.randint(0, n_classes, (E, n_qpts), generator=g)
    desc = torch.zeros(E, 32, dtype=torch.int32)
    desc[:, ops.HD_N_PROTO] = torch.tensor(n_proto, dtype=torch.int32)
    desc = desc.cuda()
    G = ops.ce_grad(Z.reshape(-1, 4).cuda(), desc.view(-1)[ops.HD_N_PROTO:], 32, E, n_cap, n_qpts, n_classes, labels.cuda(),
                    torch.tensor(gscale, device="cuda"))
    G = G.view(planes, E, n_cap, 4).cpu()
    errs, e32 = {"G": 0.0}, {"G": 0.0}
    for e in range(E):
        Ze, Ge = torch.cat(list(Z[:, e]), 1), torch.cat(list(G[:, e]), 1)
        want = R.ce_grad64(Ze, n_proto[e], labels[e], n_classes, gscale)
        errs["G"] = max(errs["G"], R.rel(Ge, want))
        e32["G"] = max(e32["G"], R.rel(R.ce_grad64(Ze, n_proto[e], labels[e], n_classes, gscale, dtype=torch.float32), want))
        assert torch.equal(Ge == 0, want == 0), "exact zeros (rows outside the query rows, columns >= n_classes)"
        assert (Ge[:n_proto[e]] == 0).all() and (Ge[n_proto[e] + n_qpts:] == 0).all()
    _hold("D n_classes=%d" % n_classes, errs, e32, BAR)


# ----------------------------------------------------------------------------------------------------------------------
# E: prototypes, forward and backward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_launch", [True, False])
@pytest.mark.parametrize("n_way,k_shot,seg_counts", [(2, 2, ((3, 10), (11, 40))), (4, 1, ((3, 10, 11, 40), (40, 11, 10, 3)))])
@pytest.mark.parametrize("D", [64, 132, 256])
def test_prototypes_forward_and_backward(ops, D, n_way, k_shot, seg_counts, one_launch):
    """E.  r3d_head_prototypes_batched then r3d_head_prototypes_bwd_batched, E = 2 with different masks: foreground
    segments of 3, 10, 11 and 40 points at k = 10 (n < k and n == k: identity; n == k + 1: the first FPS; n > k), both FPS
    forms (the persistent launch has its own occupancy path above D = 192).  Forward: nodes against float64 cluster means,
    cluster_count, desc.  Backward: dsfeat, dqfeat against float64 autograd of sum(nodes * R), both views of ONE
    gradient matrix of leading dimension D + 4 whose padding columns stay untouched.
    measured: nodes 4.6e-8 (e32 6.9e-8)  dsfeat 2.1e-8 (e32 1.1e-8)  dqfeat 0 (a copy)."""
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    E, N, k_sub, n_q = 2, 128, 10, 1
    S = n_way * k_shot
    ep_rows = (S + n_q) * N
    g = torch.Generator().manual_seed(D + n_way)
    feat = torch.randn(E * ep_rows, D, generator=g) * 0.1
    ys = [_masks(n_way, k_shot, N, seg_counts[e], 10 * e + n_way) for e in range(E)]
    hb = ops.HeadBuffers(n_way, k_shot, N, n_q * N, k_sub, 8, D, "cuda", E=E)
    hb.fps_one_launch = one_launch
    hb.nodes.fill_(7.0)
    fd = feat.cuda()
    sy = torch.stack(ys).reshape(E, S, N).to(torch.int32).contiguous().cuda()
    ops.head_prototypes(hb, sy, None, fd, fd[S * N:], ep_rows)
    Rm = torch.randn(E * hb.n_cap, D, generator=g)
    PAD = 123.0
    dfeat = torch.full((E * ep_rows, D + 4), PAD, device="cuda")
    dfeat.view(E, ep_rows, D + 4)[:, :S * N, :D].zero_()  # (the support rows start at zero: points in no list keep it)
    Rd = Rm.cuda()
    _lib.check(lib.r3d_head_prototypes_bwd_batched(
        E, ops._p(Rd), D, hb.n_cap, n_way, k_shot, N, D, n_q * N, ops._p(hb.desc), 32, ops._p(hb.assign), 2 * S * N,
        ops._p(hb.cluster_count), hb.n_cap, ops._p(hb.proto_ws), hb.proto_stride, ops._p(dfeat), D + 4, ep_rows,
        ops._p(dfeat[S * N:]), D + 4, ep_rows, ops._st()))
    torch.cuda.synchronize()
    desc = hb.desc.view(E, 32).cpu()
    nodes, cc = hb.nodes.view(E, hb.n_cap, D).cpu(), hb.cluster_count.view(E, hb.n_cap).cpu()
    dfeat = dfeat.view(E, ep_rows, D + 4).cpu()
    errs = dict(nodes=0.0, dsfeat=0.0, dqfeat=0.0)
    e32 = dict(errs)
    for e in range(E):
        f = feat[e * ep_rows:(e + 1) * ep_rows]
        want, counts, seg_m, sl, ql = R.proto_nodes(f[:S * N], f[S * N:], ys[e], k_sub)
        n_proto, n = sum(seg_m), want.shape[0]
        assert seg_m[1:] == [c if c <= k_sub else O.fps_sample_count(c, k_sub) for c in seg_counts[e]]
        assert desc[e, ops.HD_SEG_COUNT:ops.HD_SEG_COUNT + n_way + 1].tolist() == [S * N - sum(seg_counts[e])] + list(seg_counts[e])
        assert desc[e, ops.HD_SEG_M:ops.HD_SEG_M + n_way + 1].tolist() == seg_m
        assert desc[e, ops.HD_SEG_POFF:ops.HD_SEG_POFF + n_way + 1].tolist() == [sum(seg_m[:s]) for s in range(n_way + 1)]
        assert desc[e, ops.HD_N_PROTO] == n_proto and desc[e, ops.HD_N_NODES] == n and desc[e, ops.HD_FPS_TIMEOUT] == 0
        assert torch.equal(cc[e, :n_proto].long(), counts)
        assert torch.equal(nodes[e, n_proto:n], f[S * N:])  # query rows: copies
        (want * Rm[e * hb.n_cap:e * hb.n_cap + n].double()).sum().backward()
        w32, _, _, s32, q32 = R.proto_nodes(f[:S * N], f[S * N:], ys[e], k_sub, dtype=torch.float32)
        (w32 * Rm[e * hb.n_cap:e * hb.n_cap + n]).sum().backward()
        for k, got, ref, r32 in (("nodes", nodes[e, :n_proto], want[:n_proto].detach(), w32[:n_proto].detach()),
                                 ("dsfeat", dfeat[e, :S * N, :D], sl.grad, s32.grad),
                                 ("dqfeat", dfeat[e, S * N:, :D], ql.grad, q32.grad)):
            errs[k] = max(errs[k], R.rel(got, ref))
            e32[k] = max(e32[k], R.rel(r32, ref))
        assert (dfeat[e, :, D:] == PAD).all(), "padding columns written"
        assert torch.equal(dfeat[e, :S * N, :D] == 0, sl.grad == 0)
    _hold("E D=%d %d-way %d-shot one_launch=%d" % (D, n_way, k_shot, one_launch), errs, e32, BAR)


# ----------------------------------------------------------------------------------------------------------------------
# F: contrastive loss, forward and backward
# ----------------------------------------------------------------------------------------------------------------------
# foreground points per shot: 1 (identity), 4 (its boundary), 5 (the first FPS), 60 (ordinary); support_flag per shot.
# noisy: way 0 is mixed (that is what selects the branch), and every label of a way is carried by at least two prototypes
# so that every anchor has a positive (a label held by ONE one-point shot would make the reference itself 0 / 0)
_CT = {
    (2, "clean"): dict(fg=((1, 60), (4, 5), (5, 1)), flag=((1, 1), (1, 1), (1, 1))),
    (5, "clean"): dict(fg=((1, 4, 5, 60, 1), (60, 1, 4, 5, 4), (5, 1, 60, 4, 1)), flag=((1,) * 5,) * 3),
    (2, "noisy"): dict(fg=((4, 60), (1, 5), (5, 60)), flag=((1, 0), (1, 1), (0, 1))),
    (5, "noisy"): dict(fg=((1, 4, 5, 60, 1), (60, 1, 4, 5, 4), (5, 1, 60, 4, 1)),
                       flag=((1, 0, 1, 0, 1), (0, 0, 0, 0, 1), (1, 1, 0, 1, 1))),
}


@pytest.mark.parametrize("branch", ["clean", "noisy"])
@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("n_way", [2, 3])
@pytest.mark.parametrize("k_shot", [2, 5])
@pytest.mark.parametrize("D", [64, 132, 256])
def test_contrast_forward_and_backward(ops, D, k_shot, n_way, E, branch):
    """F.  r3d_contrast_fwd / _bwd (contrast.contrast_forward / contrast_backward), gscale 0.1: shots of 1, 4, 5 and 60
    foreground points, the clean branch (two negative shots of the next way) and the noisy branch (labels = the flags),
    the D-strided tables at three widths; loss, dfeat, dW, db against supcon64 (dW, db summed over the batch).
    Background rows and query rows of dfeat exactly zero.
    measured, worst of the 48 cases: loss 1.1e-7 (e32 5.0e-8)  dfeat 2.9e-6 (e32 4.1e-7)  dW 2.4e-6 (e32 4.8e-7)
    db 2.3e-6 (e32 6.8e-7)."""
    from r3dfsseg_amd import contrast
    N, gscale = 128, 0.1
    S = n_way * k_shot
    ep_rows = (S + 1) * N  # one query cloud behind the support rows
    t = _CT[(k_shot, branch)]
    g = torch.Generator().manual_seed(D + 7 * k_shot + n_way)
    feat = torch.randn(E * ep_rows, D, generator=g) * 0.1
    W, b = torch.randn(128, D, generator=g) / D ** 0.5, torch.randn(128, generator=g) * 0.1
    flag = torch.tensor(t["flag"][:n_way])
    ys = []
    for e in range(E):
        rs = np.random.RandomState(100 * e + D)
        y = torch.zeros(n_way, k_shot, N, dtype=torch.int64)
        for w in range(n_way):
            for k in range(k_shot):
                c = t["fg"][w][k]
                c = {4: 5, 5: 4}.get(c, c) if e == 1 else c  # (episode 1: other masks, 4 <-> 5 swapped)
                y[w, k, torch.from_numpy(rs.permutation(N)[:c])] = 1
        ys.append(y)
    model = SimpleNamespace(n_way=n_way, k_shot=k_shot, n_points=N, feat_dim=D)
    fd = feat.cuda()
    loss, saved = contrast.contrast_forward(model, fd, W.cuda(), b.cuda(), torch.stack(ys).cuda(),
                                            torch.stack([flag] * E).cuda(), E, ep_rows)
    dfeat, dW, db = contrast.contrast_backward(saved, torch.tensor(gscale, device="cuda"), E * ep_rows)
    torch.cuda.synchronize()
    loss, dfeat, dW, db = loss.cpu(), dfeat.view(E, ep_rows, D).cpu(), dW.cpu(), db.cpu()
    ref = {64: dict(dW=0, db=0), 32: dict(dW=0, db=0)}
    errs = dict(closs=0.0, cdfeat=0.0)
    e32 = dict(errs)
    for e in range(E):
        f = feat[e * ep_rows:e * ep_rows + S * N]
        res = {}
        for bits, dt in ((64, torch.float64), (32, torch.float32)):
            l, sl, Wl, bl = R.supcon64(W, b, f, ys[e], flag, dtype=dt)
            assert torch.isfinite(l), "the reference itself is not finite: an anchor without a positive"
            (gscale * l).backward()
            res[bits] = (l.detach(), sl.grad)
            ref[bits]["dW"] = ref[bits]["dW"] + Wl.grad
            ref[bits]["db"] = ref[bits]["db"] + bl.grad
        errs["closs"] = max(errs["closs"], abs(loss[e].item() - res[64][0].item()) / abs(res[64][0].item()))
        e32["closs"] = max(e32["closs"], abs(res[32][0].item() - res[64][0].item()) / abs(res[64][0].item()))
        errs["cdfeat"] = max(errs["cdfeat"], R.rel(dfeat[e, :S * N], res[64][1]))
        e32["cdfeat"] = max(e32["cdfeat"], R.rel(res[32][1], res[64][1]))
        assert (dfeat[e, S * N:] == 0).all(), "query rows"
        assert (dfeat[e, :S * N].view(n_way, k_shot, N, D)[ys[e] == 0] == 0).all(), "background rows"
    errs.update(cdW=R.rel(dW, ref[64]["dW"]), cdb=R.rel(db, ref[64]["db"]))
    e32.update(cdW=R.rel(ref[32]["dW"], ref[64]["dW"]), cdb=R.rel(ref[32]["db"], ref[64]["db"]))
    _hold("F D=%d %d-shot %d-way E=%d %s" % (D, k_shot, n_way, E, branch), errs, e32, BAR)


# ----------------------------------------------------------------------------------------------------------------------
# G: one chain
# ----------------------------------------------------------------------------------------------------------------------
def test_one_chain_at_output_dim_128(ops):
    """G.  head_train.lp_forward + lp_backward on a model with output_dim = 128 (D = 256), 4 ways x 2 shots of 128 points,
    10 sub-prototypes, k_connect 20, E = 2, random 0.08-scale features: loss and dfeat against the float64 chain
    prototypes -> label propagation -> cross entropy (references 3 -> 1 -> 2), the device's neighbour lists injected
    after they have been checked against the oracle's.
    measured: loss 1.3e-6 (e32 2.5e-8: one scalar, 11 ulp of fp32)  dfeat 8.9e-6 (e32 5.8e-6)."""
    from r3dfsseg_amd import head_train, synthetic as Sy
    from r3dfsseg_amd.mpti import MPTI_SelfAtten
    n_way, k_shot, N, E = 4, 2, 128, 2
    cfg = Sy.make_cfg(n_way=n_way, k_shot=k_shot, pc_npts=N, n_subprototypes=10, k_connect=20, output_dim=128, lp_max_iter=300,
                      lp_tol=TOL)
    m = MPTI_SelfAtten(SimpleNamespace(**cfg)).cuda().train()
    D, S = m.feat_dim, n_way * k_shot
    assert D == 256
    eps = [Sy.make_episode(cfg, 20 + e, train=True)[0] for e in range(E)]
    sy, qy = torch.stack([d[1] for d in eps]), torch.stack([d[3] for d in eps])
    n_q = qy.shape[1]
    ep_rows = (S + n_q) * N
    feat = torch.randn(E * ep_rows, D, generator=torch.Generator().manual_seed(3)) * 0.08
    fd = feat.cuda()
    m._lp_force = True  # the full CG budget and the exact neighbour kernel
    m._trace = {}
    loss, logits, pred, saved = head_train.lp_forward(m, fd, fd[S * N:], sy.cuda(), qy.cuda(), E, ep_rows)
    dfeat = head_train.lp_backward(saved, torch.ones((), device="cuda"))
    torch.cuda.synchronize()
    assert m.lp_converged(backward=True)
    hb = saved.hb
    assert hb.planes == 2
    desc = hb.desc.view(E, 32).cpu()
    nbr = m._trace["nbr"].view(E, hb.n_cap, hb.kp1).cpu().to(torch.int64)
    nodes = hb.nodes.view(E, hb.n_cap, D).cpu()
    loss, dfeat = loss.cpu(), dfeat.view(E, ep_rows, D).cpu()
    errs = dict(chain_loss=0.0, chain_dfeat=0.0)
    e32 = dict(errs)
    for e in range(E):
        f = feat[e * ep_rows:(e + 1) * ep_rows]
        res = {}
        for bits, dt in ((64, torch.float64), (32, torch.float32)):
            nd, _, seg_m, sl, ql = R.proto_nodes(f[:S * N], f[S * N:], sy[e], 10, dtype=dt)
            n_proto, n = sum(seg_m), nd.shape[0]
            if bits == 64:
                assert desc[e, ops.HD_N_PROTO] == n_proto and desc[e, ops.HD_N_NODES] == n
                assert torch.equal(nbr[e, :n], O.knn_l2(nodes[e, :n], hb.kp1)), "neighbour lists differ from the oracle's"
            Y = torch.zeros(n, n_way + 1)
            row = 0
            for s, ms in enumerate(seg_m):
                Y[row:row + ms, s] = 1
                row += ms
            _, Z = R.lp_from_nodes(nd, nbr[e, :n], Y, m.sigma, ALPHA)  # reference 1 on the nodes of reference 3
            l = torch.nn.functional.cross_entropy(Z[n_proto:], qy[e].reshape(-1))
            Z.backward(R.ce_grad64(Z.detach(), n_proto, qy[e], n_way + 1, 1.0, dtype=dt))  # reference 2
            res[bits] = (l.detach(), torch.cat((sl.grad, ql.grad), 0))
        errs["chain_loss"] = max(errs["chain_loss"], abs(loss[e].item() - res[64][0].item()) / abs(res[64][0].item()))
        e32["chain_loss"] = max(e32["chain_loss"], abs(res[32][0].item() - res[64][0].item()) / abs(res[64][0].item()))
        errs["chain_dfeat"] = max(errs["chain_dfeat"], R.rel(dfeat[e], res[64][1]))
        e32["chain_dfeat"] = max(e32["chain_dfeat"], R.rel(res[32][1], res[64][1]))
    _hold("G chain D=256 E=2", errs, e32, BAR)
