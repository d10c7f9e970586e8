"""The CG's LDS-resident SpMV (csrc/head_graph.hip: r3d_cg_spmv_lds_kernel) on graphs whose row lengths are CHOSEN:
neighbour lists are injected into ops.label_propagate and the adjoint, so hub rows of two and three 384-entry chunks, a
row of exactly 384 and one of exactly 385 entries, short rows, node counts that are no multiple of 4 or 128 and whole
empty trailing row blocks are all there by construction -- and every case reads the CSR back and asserts it.

The kernel runs one resident round (a workgroup walks several 4-row groups, in passes of 64 rows per wave) and streams the
matrix as (row, chunk) items ahead of the gather.  How the bytes arrive is free, the arithmetic is not: it must give the
bits of the row-per-wave form r3d_cg_spmv_kernel, and the closed form of the reference within the bar of
test_gpu_head.py::test_label_propagation_vs_closed_form."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import head_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4       # the bar of test_label_propagation_vs_closed_form: max |Z - Z64| <= TOL * max(1, max |Z64|)
ALPHA, CG_TOL, ITERS = 0.99, 1e-6, 300
D, K = 64, 8     # feature width, neighbours per node (kp1 = 9)
N_PROTO = 60
LDS, ROW_PER_WAVE = 0, 1 << 30  # r3d_debug_set_cg_spmv_lds_min_blocks: always / never the LDS form


@pytest.fixture(scope="module")
def ops():
    from r3dfsseg_amd import ops as _ops
    from r3dfsseg_amd import _lib
    _lib.load()
    return _ops


def _lists(n):
    """Neighbour lists (n, K + 1) int64, column 0 = the node itself (dropped by the op), and the row lengths of the
    symmetrised graph they give.  Three hubs are listed by everyone (rows of n - 1 entries); node A is listed by 381 plain
    nodes and lists the hubs (384 entries), node B by 382 (385 entries); a plain node lists the hubs, its three successors
    on a ring of the plain nodes and, the first 381 / 382 of them, A / B: 11 entries at the most.  Unused slots hold the
    node itself (the diagonal is dropped)."""
    hubs, A, B = [7, n // 2, n - 1], 129, n - 3
    special = set(hubs + [A, B])
    assert len(special) == 5
    plain = [i for i in range(n) if i not in special]
    P = len(plain)
    assert P >= 382 + 3
    nbr = np.empty((n, K + 1), dtype=np.int64)
    nbr[:, 0] = np.arange(n)
    for h in hubs:
        nbr[h, 1:] = [o for o in hubs if o != h] + [h] * (K - 2)
    for s in (A, B):
        nbr[s, 1:] = hubs + [s] * (K - 3)
    for p, i in enumerate(plain):
        nbr[i, 1:] = hubs + [plain[(p + 1) % P], plain[(p + 2) % P], plain[(p + 3) % P], A if p < 381 else i, B if p < 382 else i]
    adj = np.zeros((n, n), dtype=bool)
    adj[np.repeat(np.arange(n), K), nbr[:, 1:].reshape(-1)] = True
    adj |= adj.T
    adj[np.arange(n), np.arange(n)] = False
    rowlen = adj.sum(1)
    assert all(rowlen[h] == n - 1 for h in hubs) and rowlen[A] == 384 and rowlen[B] == 385
    assert rowlen[[i for i in plain]].max() <= 16
    return torch.from_numpy(nbr), rowlen, hubs


def _features(n, seed):
    x, lab = R.graph_nodes(N_PROTO, n - N_PROTO, D, seed)
    Y = torch.zeros(n, 4)
    Y[torch.arange(N_PROTO), lab[:N_PROTO]] = 1
    return x, Y


def _buffers(ops, n_cap_nodes, E):
    """HeadBuffers of E systems with room for n_cap_nodes nodes (and three spare prototype slots)."""
    k_sub = N_PROTO // 3 + 2
    hb = ops.HeadBuffers(2, 1, n_cap_nodes - N_PROTO, n_cap_nodes - N_PROTO, k_sub, K, D, "cuda", E=E)
    assert hb.n_cap > n_cap_nodes and hb.kp1 == K + 1
    return hb


def _load(ops, hb, systems):
    """systems: per system (x, Y, nbr).  Rows beyond n: 7.0 in the node matrix, -1 in the lists."""
    E, nc = hb.E, hb.n_cap
    desc = hb.desc.view(E, 32)
    hb.nodes.fill_(7.0)
    hb.Y.zero_()
    nbr = torch.full((E, nc, hb.kp1), -1, dtype=torch.int32)
    for e, (x, Y, nb) in enumerate(systems):
        n = x.shape[0]
        hb.nodes[e * nc:e * nc + n] = x.cuda()
        hb.Y[e * nc:e * nc + n] = Y.cuda()
        nbr[e, :n] = nb.to(torch.int32)
        desc[e, ops.HD_N_PROTO] = N_PROTO
        desc[e, ops.HD_N_NODES] = n
    return nbr.cuda().contiguous()


def _solve(ops, hb, nbr, G, min_blocks, iters=ITERS, adjoint=True):
    """Forward (and adjoint) solve with the SpMV form `min_blocks` selects -> dict of device tensors (clones)."""
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    E, nc = hb.E, hb.n_cap
    old = lib.r3d_debug_set_cg_spmv_lds_min_blocks(min_blocks)
    try:
        hb.Z.fill_(float("nan"))
        hb.stats.zero_()
        Z = ops.label_propagate(hb, nbr, 1.0, ALPHA, iters, CG_TOL)
        out = dict(Z=Z.clone(), stats=hb.stats.clone())
        if adjoint:
            lam = torch.zeros(E * nc, 4, device="cuda")
            dnodes = torch.zeros(E * nc, D, device="cuda")
            stats_b = torch.zeros(E, 2, device="cuda", dtype=torch.int32)
            _lib.check(lib.r3d_label_propagate_bwd_batched(
                E, ops._p(hb.nodes), hb.nodes.stride(0), D, hb.kp1, ops._p(Z), ops._p(G), ops._p(hb.n_nodes_ptr()), 32, nc, 1.0,
                ALPHA, iters, CG_TOL, ops._p(lam), ops._p(dnodes), D, ops._p(hb.lp_ws), hb.lp_words, hb.lp_stride,
                ops._p(stats_b), 2, ops._st()))
            out.update(lam=lam, dnodes=dnodes, stats_bwd=stats_b)
        torch.cuda.synchronize()
    finally:
        lib.r3d_debug_set_cg_spmv_lds_min_blocks(old)
    return out


def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


def _check_csr(hb, e, n, rowlen, hubs):
    """The CSR the op built has the row lengths the lists were written for."""
    n_got, row_ptr, col, val = hb.csr(e)
    got = (row_ptr[1:] - row_ptr[:-1]).cpu().numpy()
    assert n_got == n and np.array_equal(got, rowlen), "system %d: row lengths differ from the lists'" % e
    assert sorted(np.nonzero(got > 16)[0].tolist()) == sorted(hubs + [129, n - 3])
    assert got[129] == 384 and got[n - 3] == 385                                     # one chunk exactly / one entry more
    assert all((got[h] + 383) // 384 == (2 if n < 769 else 3) for h in hubs)         # hub rows: two / three chunks
    return got


NS = (521, 899, 777)  # no multiple of 4 or 128; 521 leaves the 128-row blocks from row 640 on empty in a capacity of 900+


@pytest.fixture(scope="module")
def three(ops):
    """Three systems of different size in one batch, solved forward and adjoint with both SpMV forms (the LDS form twice),
    and their float64 closed forms: computed once for the tests below."""
    systems, meta = [], []
    for e, n in enumerate(NS):
        nbr, rowlen, hubs = _lists(n)
        x, Y = _features(n, 11 + e)
        systems.append((x, Y, nbr))
        meta.append((n, rowlen, hubs))
    hb = _buffers(ops, max(NS), len(NS))
    nbr = _load(ops, hb, systems)
    G = torch.randn(len(NS) * hb.n_cap, 4, generator=torch.Generator().manual_seed(5)).cuda()
    runs = {name: _solve(ops, hb, nbr, G, mb) for name, mb in (("lds", LDS), ("rpw", ROW_PER_WAVE), ("lds2", LDS))}
    csr = [_check_csr(hb, e, *meta[e]) for e in range(len(NS))]
    ref = []
    with torch.no_grad():
        for e, (x, Y, nb) in enumerate(systems):
            n = x.shape[0]
            S, Z = R.lp_from_nodes(x.double(), nb, Y, 1.0, ALPHA)
            Ge = G[e * hb.n_cap:e * hb.n_cap + n].cpu().double()
            lam = torch.linalg.inv(torch.eye(n, dtype=torch.float64) - ALPHA * S + R.EPS) @ Ge
            ref.append((Z, lam))
    return SimpleNamespace(hb=hb, runs=runs, meta=meta, csr=csr, ref=ref, systems=systems)


def test_the_batch_has_the_shape_it_was_chosen_for(three):
    """Node counts inside one capacity, none a multiple of 4 or of 128, one leaving whole trailing 128-row blocks empty;
    hub rows of two chunks at 521 and three at 777 and 899, rows of exactly 384 and 385 entries, the rest <= 16."""
    nc = three.hb.n_cap
    assert all(n % 4 and n % 128 and n < nc for n in NS)
    assert (nc + 127) // 128 - (min(NS) + 127) // 128 >= 2
    for (n, rowlen, hubs), got in zip(three.meta, three.csr):
        assert (np.sort(got)[:-5] <= 16).all() and np.sort(got)[-3:].tolist() == [n - 1] * 3


def test_streamed_lds_form_gives_the_bits_of_the_row_per_wave_form(three):
    """Z, lam, dnodes and both stats words (iterations included), forward and adjoint: LDS form == row-per-wave form, and
    two runs of the LDS form agree."""
    for k in ("stats", "stats_bwd"):
        st = three.runs["lds"][k].view(-1, 2).cpu()
        print("CGS| %s (converged, iterations) per system: %s" % (k, st.tolist()))
        assert (st[:, 0] == 1).all() and (st[:, 1] > 2).all(), "%s: a solve did not converge %s" % (k, st.tolist())
    _same_bits(three.runs["lds"], three.runs["rpw"], "LDS form against row-per-wave form")
    _same_bits(three.runs["lds"], three.runs["lds2"], "LDS form, second run")
    assert torch.isfinite(three.runs["lds"]["dnodes"]).all()


def test_streamed_lds_form_against_the_closed_form(three):
    """Forward and adjoint solutions of the LDS form against the dense float64 closed form inv(I - alpha S) of the
    reference on the same lists, at the bar of test_label_propagation_vs_closed_form."""
    nc = three.hb.n_cap
    for e, n in enumerate(NS):
        Zw, lamw = three.ref[e]
        for name, got, want in (("Z", three.runs["lds"]["Z"], Zw), ("lam", three.runs["lds"]["lam"], lamw)):
            g = got[e * nc:e * nc + n].cpu().double()
            scale = want.abs().max().item()
            err = (g - want).abs().max().item()
            print("CGS| system %d (n %d) %-3s err %.2e  max|ref| %.2e" % (e, n, name, err, scale))
            assert err <= TOL * max(1.0, scale), (e, name, err, scale)


@pytest.mark.parametrize("E", [1, 40, 150, 600])
def test_launch_sizes(ops, E):
    """E = 1 with the LDS form forced: fewer workgroups than the chip holds.  E = 40 systems of 521 nodes (five 128-row
    blocks each): the resident slots are shared out among the systems, one workgroup per block.  E = 150: at two
    resident workgroups per CU (512 slots) three workgroups per system, each walking more than 128 rows.  E = 600: fewer
    than two slots per system at any occupancy (256 CUs hold at most 4 workgroups of 512 threads each = 1024, and a
    system never gets less than one): ONE workgroup per system, which takes the system's 133 4-row groups in two passes.
    The systems share their lists and differ in their features.  Same bits as the row-per-wave form, every system."""
    n = 521
    nbr, rowlen, hubs = _lists(n)
    x, Y = _features(n, 3)
    g = torch.Generator().manual_seed(E)
    systems = [(x + 1e-3 * torch.randn(x.shape, generator=g), Y, nbr) for _ in range(E)]
    hb = _buffers(ops, n, E)
    nb = _load(ops, hb, systems)
    a = _solve(ops, hb, nb, None, LDS, iters=60, adjoint=False)
    for e in sorted({0, E // 2, E - 1}):
        _check_csr(hb, e, n, rowlen, hubs)
    b = _solve(ops, hb, nb, None, ROW_PER_WAVE, iters=60, adjoint=False)
    st = a["stats"].view(-1, 2).cpu()
    assert (st[:, 0] == 1).all() and (st[:, 1] > 2).all(), st.tolist()
    _same_bits(a, b, "E = %d" % E)
    assert torch.isfinite(a["Z"].view(E, hb.n_cap, 4)[:, :n]).all()
