"""The CG iteration in one launch (csrc/head_graph.hip: r3d_cg_spmv_lds_kernel with the update of the iteration before
folded into its head).  Launch j > 0 of a solve forms alpha, x and the new residual itself, its workgroups hand their
block partials to the one that arrives last, and all of them wait INSIDE the launch for the coefficients that one
publishes as tagged words.  None of that may change a bit: every case here is compared with the row-per-wave form
(r3d_cg_spmv_kernel + r3d_cg_update_kernel, two launches per iteration), which shares no hand-off with it.

Graphs, features and buffers are those of test_gpu_cg_spmv_stream.py (chosen row lengths; n = 521 / 777 / 899 in a capacity
of 900+).  Before every solve the whole scratch -- the tagged words, tickets and partials of the solve before included --
is read once with plain loads, so that no stale copy of a polled line is cold by accident."""
import pytest
import torch

import test_gpu_cg_spmv_stream as H

pytestmark = pytest.mark.gpu

LDS, RPW = H.LDS, H.ROW_PER_WAVE
ITERS = 120


@pytest.fixture(scope="module")
def ops():
    from r3dfsseg_amd import ops as _ops
    from r3dfsseg_amd import _lib
    _lib.load()
    return _ops


def _systems(ns, zero_rhs=()):
    out = []
    for e, n in enumerate(ns):
        nbr, _, _ = H._lists(n)
        x, Y = H._features(n, 11 + e)
        out.append((x, torch.zeros_like(Y) if e in zero_rhs else Y, nbr))
    return out


def _solve(ops, hb, nbr, G, form, iters=ITERS, adjoint=True):
    hb.lp_ws.sum().item()  # plain loads of every line a solve before this one left behind
    return H._solve(ops, hb, nbr, G, form, iters=iters, adjoint=adjoint)


def _stats(run, key="stats"):
    return run[key].view(-1, 2).cpu()


@pytest.fixture(scope="module")
def batch(ops):
    """Four systems in one batch (n = 521, 899, 777, 521 with other features), buffers, lists and a cotangent."""
    ns = H.NS + (521,)
    systems = _systems(ns)
    hb = H._buffers(ops, max(ns), len(ns))
    nbr = H._load(ops, hb, systems)
    G = torch.randn(len(ns) * hb.n_cap, 4, generator=torch.Generator().manual_seed(5)).cuda()
    return hb, nbr, G, systems


def test_systems_that_converge_at_different_iterations(ops, batch):
    """One batch whose systems stop at different iterations: launches that hold live and finished systems side by side,
    the exit of a system that has just converged (its last x update, the residual it leaves) and the closing update."""
    hb, nbr, G, _ = batch
    a = _solve(ops, hb, nbr, G, LDS)
    b = _solve(ops, hb, nbr, G, RPW)
    for key in ("stats", "stats_bwd"):
        st = _stats(a, key)
        print("CGF| %s (converged, iterations): %s" % (key, st.tolist()))
        assert (st[:, 0] == 1).all() and (st[:, 1] > 2).all() and (st[:, 1] < ITERS).all(), st.tolist()
        assert len(set(st[:, 1].tolist())) > 1, "%s: every system took %d iterations" % (key, st[0, 1])
    H._same_bits(a, b, "one launch per iteration against two")


@pytest.mark.parametrize("budget", [1, 2, 5])
def test_budget_exhausted(ops, batch, budget):
    """max_iter launches and no convergence: the stats say so, the count is the budget, Z has the bits of the other form."""
    hb, nbr, G, _ = batch
    a = _solve(ops, hb, nbr, G, LDS, iters=budget)
    b = _solve(ops, hb, nbr, G, RPW, iters=budget)
    for key in ("stats", "stats_bwd"):
        st = _stats(a, key)
        assert (st[:, 0] == 0).all() and (st[:, 1] == budget).all(), (key, st.tolist())
    H._same_bits(a, b, "budget %d" % budget)
    assert torch.isfinite(a["Z"].view(hb.E, hb.n_cap, 4)[:, :521]).all()


def test_zero_right_hand_side_in_one_system(ops):
    """System 1 of three has Y = 0 (converged before the first iteration); the others carry zero label COLUMNS as every
    episode does (<p, q> = 0 there: alpha and beta take their guarded value 0)."""
    systems = _systems(H.NS, zero_rhs=(1,))
    hb = H._buffers(ops, max(H.NS), len(H.NS))
    nbr = H._load(ops, hb, systems)
    assert (hb.Y.view(hb.E, hb.n_cap, 4)[0, :, 3] == 0).all() and (hb.Y.view(hb.E, hb.n_cap, 4)[0, :, 0] != 0).any()
    G = torch.randn(len(H.NS) * hb.n_cap, 4, generator=torch.Generator().manual_seed(6)).cuda()
    G.view(hb.E, hb.n_cap, 4)[2].zero_()  # ... and the adjoint of system 2 has a zero right-hand side
    a = _solve(ops, hb, nbr, G, LDS)
    b = _solve(ops, hb, nbr, G, RPW)
    st, stb = _stats(a), _stats(a, "stats_bwd")
    assert st[:, 0].tolist() == [1, 1, 1] and st[1, 1] == 0 and st[0, 1] > 2 and st[2, 1] > 2, st.tolist()
    assert stb[:, 0].tolist() == [1, 1, 1] and stb[2, 1] == 0 and stb[0, 1] > 2, stb.tolist()
    n1, n2 = H.NS[1], H.NS[2]
    assert (a["Z"].view(hb.E, hb.n_cap, 4)[1, :n1] == 0).all() and (a["lam"].view(hb.E, hb.n_cap, 4)[2, :n2] == 0).all()
    H._same_bits(a, b, "zero right-hand side")


def test_the_same_scratch_again_and_after_another_batch(ops, batch):
    """Forward, adjoint, forward on one scratch; then a solve of TWO of the systems on the same memory (other ticket counts,
    other tags left behind), then all four again: tags and tickets of an earlier solve must not count for a later one."""
    hb, nbr, G, systems = batch
    first = _solve(ops, hb, nbr, G, LDS)                       # forward, adjoint
    third = _solve(ops, hb, nbr, G, LDS, adjoint=False)        # forward again
    assert torch.equal(third["Z"], first["Z"]) and torch.equal(third["stats"], first["stats"])
    hb2 = H._buffers(ops, max(H.NS), 2)
    assert hb2.n_cap == hb.n_cap and hb2.lp_stride == hb.lp_stride
    nbr2 = H._load(ops, hb2, systems[2:])
    ref2 = _solve(ops, hb2, nbr2, None, RPW, iters=7, adjoint=False)   # (7: stops in the middle, nothing converged)
    hb2.lp_ws = hb.lp_ws                                               # the first two systems' scratch of the batch of four
    got2 = _solve(ops, hb2, nbr2, None, LDS, iters=7, adjoint=False)
    H._same_bits(got2, ref2, "two systems on the scratch of four")
    assert (_stats(got2)[:, 0] == 0).all()
    again = _solve(ops, hb, nbr, G, LDS)
    H._same_bits(again, first, "after a solve of another batch on the same scratch")


def test_captured_solve_replayed_with_other_labels(ops, batch):
    """The solve frozen into a graph and replayed three times, Y changed in between: every replay equals the eager solve
    of that Y (nothing a replay needs may live in a launch argument that changes from solve to solve)."""
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    hb, nbr, _, _ = batch
    Y0 = hb.Y.clone()
    Ys = [Y0, Y0.flip(1).contiguous(), (0.5 * Y0 + 0.25 * Y0.roll(1, 1)).contiguous()]
    want = []
    for Y in Ys:
        hb.Y.copy_(Y)
        want.append(_solve(ops, hb, nbr, None, RPW, adjoint=False))
    old = lib.r3d_debug_set_cg_spmv_lds_min_blocks(LDS)
    try:
        hb.Y.copy_(Y0)
        ops.label_propagate(hb, nbr, 1.0, H.ALPHA, ITERS, H.CG_TOL)  # (one-time host set-up stays out of the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.label_propagate(hb, nbr, 1.0, H.ALPHA, ITERS, H.CG_TOL)
    finally:
        lib.r3d_debug_set_cg_spmv_lds_min_blocks(old)
    try:
        for i in (1, 2, 0):
            hb.Y.copy_(Ys[i])
            hb.Z.fill_(float("nan"))
            hb.stats.zero_()
            hb.lp_ws.sum().item()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(hb.stats, want[i]["stats"]), (i, hb.stats.tolist(), want[i]["stats"].tolist())
            assert torch.equal(hb.Z, want[i]["Z"]), "replay with labels %d differs from the eager solve" % i
    finally:
        hb.Y.copy_(Y0)


def test_one_system_with_more_workgroups_than_update_blocks(ops):
    """E = 1 with the LDS form forced: one workgroup per 128 rows, twice as many as there are 256-row blocks of the
    update's partition -- half the workgroups have no block and only take their ticket."""
    n = 521
    systems = _systems((n,))
    hb = H._buffers(ops, max(H.NS), 1)
    assert (hb.n_cap + 127) // 128 >= 2 * ((hb.n_cap + 255) // 256) - 1 > (hb.n_cap + 255) // 256
    nbr = H._load(ops, hb, systems)
    G = torch.randn(hb.n_cap, 4, generator=torch.Generator().manual_seed(7)).cuda()
    a = _solve(ops, hb, nbr, G, LDS)
    b = _solve(ops, hb, nbr, G, RPW)
    st = _stats(a)
    assert st[0, 0] == 1 and 2 < st[0, 1] < ITERS, st.tolist()
    H._same_bits(a, b, "E = 1")
