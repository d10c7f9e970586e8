"""Every kernel configuration of the kNN launcher (csrc/knn.hip: knn_choose) against the C oracle, bit for bit: each case
of tests/knn_path_cases.py first asserts -- with r3d_debug_knn_path, on the operands it is about to pass and the switches as
set -- that it reaches the configuration it claims, then runs ops.knn.  Indices must equal the oracle's and scores must have
the same bits; there is no tolerance anywhere in this file (the oracle defines the arithmetic and the tie order).  For L2
distances the sign convention of test_knn_l2_bitexact holds: abs(score) == the oracle's distance."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_path_cases as KC  # noqa: E402

from oracle import r3d_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from r3dfsseg_amd import ops as _ops
    from r3dfsseg_amd import _lib
    _lib.load()
    return _ops


@pytest.fixture(scope="module")
def lib():
    from r3dfsseg_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------------------------------ shared inputs and references
@functools.lru_cache(maxsize=None)
def _small_x(kind, B, C, N):
    x = torch.from_numpy(KC.small_input(kind, B, C, N))
    x.numpy().flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def _small_want(kind, B, C, N, k, mode):
    """The oracle's (indices int64, scores) of one input, computed once for every case that shares it."""
    x = _small_x(kind, B, C, N)
    if mode == "dgcnn":
        want, wsc = O.knn(x, k, return_dist=True)
        return want.numpy(), wsc.numpy()
    per = [O.knn_l2(x[b].t().contiguous(), k, return_dist=True) for b in range(B)]
    return np.stack([p[0].numpy() for p in per]), np.stack([p[1].numpy() for p in per])


def _operands(ops, case, x):
    """x (B, C, N) on the host -> (x_pm as the case's layout hands it over, x_cm or None), on the device."""
    B, C, N = x.shape
    rows = x.transpose(1, 2).reshape(B * N, C)
    if case.layout == "ld65":
        buf = torch.full((B * N, C + 1), float("nan"))
        buf[:, :C] = rows
        return buf.cuda()[:, :C], None
    if case.layout == "off4":
        buf = torch.full((B * N, C + 4), float("nan"))
        buf[:, 1:C + 1] = rows
        return buf.cuda()[:, 1:C + 1], None
    x_pm = rows.contiguous().cuda()
    return x_pm, (x.contiguous().cuda() if case.layout == "x_cm" else None)


def _run_small(ops, lib, case, x, threshold=None, filter=None, claim=None):
    """One ops.knn call of a case under its switches (or the given ones), behind the assertion of the path it takes."""
    mode = ops.SCORE_L2 if case.mode == "l2" else ops.SCORE_DGCNN
    x_pm, x_cm = _operands(ops, case, x)
    with KC.switches(lib, case.threshold if threshold is None else threshold, case.filter if filter is None else filter):
        assert ops.knn_path(x_pm, case.B, case.N, case.k, x_cm=x_cm) == (case.claim if claim is None else claim)
        got, gsc = ops.knn(x_pm, case.B, case.N, case.k, mode=mode, return_scores=True, x_cm=x_cm)
        torch.cuda.synchronize()
    return got, gsc


def _assert_is_oracle(case, got, gsc, want, wsc):
    gsc = gsc.cpu().numpy()
    if case.mode == "l2":
        gsc = np.abs(gsc)
    assert np.array_equal(gsc.view(np.int32), wsc.view(np.int32)), "%s: scores differ bitwise" % case.name
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want), "%s: indices differ" % case.name


SMALL_PARAMS = [pytest.param(c, kind, id="%s-%s" % (c.name, kind)) for c in KC.SMALL_CASES for kind in c.inputs
                if kind != "nonfinite"]


@pytest.mark.parametrize("case,kind", SMALL_PARAMS)
def test_small_k_path_is_the_oracle(ops, lib, case, kind):
    """k <= 32: plain clouds, 60 copied points per cloud (ties -> the lower index), 300 identical points in one cloud (more
    ties at the best score than the 128 survivor slots: the tile repair runs behind whichever passes the case selects),
    and the inputs that strain the bf16 bounds -- norms far above the distances, values near the bf16 subnormal range,
    channels seven decades apart.  The filter drops a neighbour SILENTLY when its upper bound falls short of tau, so on the
    bf16 cases the last three also have to equal the same call with both switches off."""
    x = _small_x(kind, case.B, case.C, case.N)
    got, gsc = _run_small(ops, lib, case, x)
    if kind in KC.STRESS and case.name in ("A", "B", "C"):
        ref, rsc = _run_small(ops, lib, case, x, threshold=0, filter=0, claim=KC.SMALL | KC.FULL)
        assert torch.equal(got, ref), "the bf16 passes changed a neighbour"
        assert torch.equal(gsc.view(torch.int32), rsc.view(torch.int32)), "the bf16 passes changed a score bit"
    _assert_is_oracle(case, got, gsc, *_small_want(kind, case.B, case.C, case.N, case.k, case.mode))


@pytest.mark.parametrize("case", [c for c in KC.SMALL_CASES if "nonfinite" in c.inputs], ids=lambda c: c.name)
def test_small_k_path_with_nonfinite_rows(ops, lib, case):
    """An infinite point and a NaN coordinate: no bound holds for them, their tiles are flagged and redone exactly.  Every
    row but the two bad QUERY rows (every score of theirs is NaN: no order) has the bits of the run with both switches
    off, and valid indices."""
    B, N = case.B, case.N
    x = _small_x("nonfinite", B, case.C, N)
    got, gsc = _run_small(ops, lib, case, x)
    ref, rsc = _run_small(ops, lib, case, x, threshold=0, filter=0, claim=KC.SMALL | KC.FULL)
    ok = torch.ones(B, N, dtype=torch.bool, device=got.device)
    for b, row in KC.NONFINITE_QUERIES:
        ok[b, row] = False
    assert int(ok.sum()) == B * N - 2
    assert torch.equal(got[ok], ref[ok]) and torch.equal(gsc[ok].view(torch.int32), rsc[ok].view(torch.int32))
    assert int(got[ok].min()) >= 0 and int(got[ok].max()) < N


# ------------------------------------------------------------------------------------------------------------- large k
@functools.lru_cache(maxsize=None)
def _large_X(kind, B, C, N, n_valid):
    X = torch.from_numpy(KC.large_input(kind, B, C, N, n_valid))
    X.numpy().flags.writeable = False
    return X


@functools.lru_cache(maxsize=None)
def _large_want(kind, B, C, N, n_valid, k):
    X = _large_X(kind, B, C, N, n_valid)
    out = []
    for b, n in enumerate(n_valid):
        want, wd = O.knn_l2(X[b, :n].contiguous(), k, return_dist=True)
        out.append((want.numpy(), wd.numpy()))
    return out


def _run_large(ops, lib, case, X):
    """-> (status word or None, indices (B, N, k), scores) of one launch over the B sets with their own counts."""
    mode = ops.SCORE_L2 if case.mode == "l2" else ops.SCORE_DGCNN
    x_pm = X.reshape(case.B * case.N, case.C).cuda()
    nv = torch.tensor(case.n_valid, dtype=torch.int32).cuda() if case.n_valid else None
    status = torch.full((1,), 0x55, dtype=torch.int32).cuda() if case.status else None  # (the call clears it itself)
    with KC.switches(lib, case.threshold, case.filter):
        assert ops.knn_path(x_pm, case.B, case.N, case.k, status=status) == case.claim
        got, gs = ops.knn(x_pm, case.B, case.N, case.k, mode=mode, n_valid=nv, n_valid_stride=1 if nv is not None else 0,
                          return_scores=True, status=status)
        torch.cuda.synchronize()
    return (None if status is None else int(status.item())), got.cpu().numpy(), gs.cpu().numpy()


def _lists_are_oracle(case, got, gs, wants):
    """Rows below each set's n_valid against the oracle on exactly those rows; rows at or beyond it are not compared."""
    for b, (want, wd) in enumerate(wants):
        n = want.shape[0]
        sc = gs[b, :n]
        if case.mode == "l2":
            sc = np.abs(sc)
        if not (np.array_equal(sc.view(np.int32), wd.view(np.int32)) and np.array_equal(got[b, :n].astype(np.int64), want)):
            return False
    return True


LARGE_PARAMS = [pytest.param(c, kind, id="%s-%s" % (c.name, kind)) for c in KC.LARGE_CASES for kind in c.inputs
                if not (kind.startswith("ties") and c.status)]


@pytest.mark.parametrize("case,kind", LARGE_PARAMS)
def test_large_k_path_is_the_oracle_per_set(ops, lib, case, kind):
    """k > 32 over sets with their OWN counts in one launch (r3d_knn_topk_batched), unsplit with the bf16 threshold pass,
    unsplit on the fp32 core, split, with C % 64 != 0, and the insertion kernel at its list lengths.  Rows at or beyond a
    set's count hold NaN or 3e38: the pack and norm kernels run over all B * N rows, and nothing a valid row gets may
    depend on them."""
    if case.mode == "dgcnn":  # (ins64: the DGCNN score form, whole sets)
        x = _small_x(kind, case.B, case.C, case.N)
        got, gsc = _run_small(ops, lib, case, x)
        _assert_is_oracle(case, got, gsc, *_small_want(kind, case.B, case.C, case.N, case.k, case.mode))
        return
    X = _large_X(kind, case.B, case.C, case.N, case.n_valid)
    status, got, gs = _run_large(ops, lib, case, X)
    assert status in (0, None), "survivor buffer overflow (status %r)" % status
    assert _lists_are_oracle(case, got, gs, _large_want(kind, case.B, case.C, case.N, case.n_valid, case.k))


@pytest.mark.parametrize("name", ["L3u", "L3s"])
def test_large_k_overflow_sets_the_status_bit(ops, lib, name):
    """The contract of the large-k streamed kernel: more exact ties at tau than a workgroup's 384 slots set status bit 0 --
    never a silently wrong list.  400 identical rows in one of 4 sets (unsplit: one workgroup sees all 400 tie at distance
    0), 800 in a single set (split: each half sees every other sub-tile, about 400 of them).  The caller's answer, the same
    call without a status word (insertion kernel), must be the oracle's."""
    case = {c.name: c for c in KC.LARGE_CASES}[name]
    kind = case.inputs[0]
    X = _large_X(kind, case.B, case.C, case.N, case.n_valid)
    wants = _large_want(kind, case.B, case.C, case.N, case.n_valid, case.k)
    status, got, gs = _run_large(ops, lib, case, X)
    if not status & 1:
        # no overflow reported: then the lists must be right, and the construction above was short, not the kernel wrong
        assert _lists_are_oracle(case, got, gs, wants), "status == %d but the lists are not the oracle's" % status
        pytest.fail("%s: %s did not overflow the survivor buffer (status %d): raise the count of identical rows"
                    % (name, kind, status))
    exact = case._replace(status=False, claim=KC.INS | ops.KNN_REGS_4)
    status2, got2, gs2 = _run_large(ops, lib, exact, X)
    assert status2 is None
    assert _lists_are_oracle(exact, got2, gs2, wants), "the insertion kernel's lists are not the oracle's"
