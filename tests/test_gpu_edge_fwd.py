"""The inference EdgeConv kernel (csrc/edgeconv.hip: r3d_edgeconv_kernel, all eight K) through r3d_edgeconv_fwd against float64:
values, EVERY max-pool winner, ties, the clamp of neighbour ids, clouds apart, refusals -- with out a column slice of a
poisoned 192-column matrix (the concat layout of the encoder) and every buffer the call writes guarded.

Reference and cases: tests/edge_fwd_ref.py (held to oracle.r3d_oracle in tests/test_edge_fwd_ref_host.py, which also shows on
the reference alone that near-ties are rare in every case).

Values: max |got - ref64| / max |ref64|, printed beside ``e32``, the figure of the same dense formula in fp32 on the CPU.
The bar is 4 x the worst figure measured on the MI355X over this module's cases (the kernel is deterministic: the margin
covers other seeds), never above CEIL = 1e-4, the bar of the older test_edgeconv_vs_oracle.

Winners: for every (point, channel), none left out, the float64 value at the device's argmax slot is within
bound = 16 * 2^-24 * (|s2| sum |W2||h1| + |t2|) of the float64 maximum (edge_fwd_ref.py says why 16)."""
import ctypes

import numpy as np
import pytest
import torch

import edge_fwd_ref as E

pytestmark = pytest.mark.gpu

CEIL = 1e-4
BAR = dict(out=1.6e-6)  # 4 x 3.81e-7 (B = 2, N = 132, K = 20; e32 3.42e-7)
assert BAR["out"] <= CEIL

POISON = 0x7FC0BEEF  # a quiet NaN of a fixed bit pattern
GUARD = 64
LDO, COL0 = 192, 64   # out = columns [64, 128) of a 192-column matrix


@pytest.fixture(scope="module")
def lib():
    from r3dfsseg_amd import _lib
    return _lib.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poisoned(n, dtype=torch.float32):
    return torch.full((n,), POISON, dtype=torch.int32, device="cuda").view(dtype)


def _call(lib, ops, B, N, K, want_argmax=True, expect_rc0=True, ldo=LDO, null=None):
    """r3d_edgeconv_fwd on device copies of ops, out a slice of a poisoned, guarded 192-column matrix, argmax guarded.
    -> (rc, out (B N, 64) host, argmax (B N, 64) host or None, untouched: nothing but the owned elements changed)."""
    M = B * N
    dev = {k: v.cuda().contiguous() for k, v in ops.items()}
    wide = _poisoned(GUARD + M * LDO + GUARD)
    out = wide[GUARD:GUARD + M * LDO].view(M, LDO)[:, COL0:COL0 + 64]
    amf = _poisoned(GUARD + M * 64 + GUARD, torch.int32)
    am = amf[GUARD:GUARD + M * 64].view(M, 64)
    ptr = {k: _p(v) for k, v in dev.items()}
    ptr["out"] = _p(out)
    if null:
        ptr[null] = None
    rc = lib.r3d_edgeconv_fwd(ptr["PQ"], ptr["idx"], ptr["W2"], ptr["s2"], ptr["t2"], ptr["out"], ldo, B, N, K,
                              _p(am) if want_argmax else None, _st())
    torch.cuda.synchronize()
    assert (rc == 0) == expect_rc0, (rc, lib.r3d_last_error_string())
    bits = wide.view(torch.int32).clone()
    owned = bits[GUARD:GUARD + M * LDO].view(M, LDO)[:, COL0:COL0 + 64]
    if rc == 0:
        assert bool((owned != POISON).all().item()), "an element of out was not written"
        owned.fill_(POISON)
    rest_ok = bool((bits == POISON).all().item())
    am_guards = bool((amf[:GUARD] == POISON).all().item() and (amf[-GUARD:] == POISON).all().item())
    am_body = bool((am == POISON).all().item())
    untouched = rest_ok and am_guards and (am_body if (rc != 0 or not want_argmax) else True)
    for k, v in dev.items():
        assert torch.equal(v.cpu(), ops[k]), "%s changed" % k
    return rc, out.cpu(), (am.cpu() if want_argmax and rc == 0 else None), untouched


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("case", E.CASES, ids=[c.name.replace(" ", "-") for c in E.CASES])
def test_values_and_every_winner(lib, case):
    """Every K at (3, 8) and (2, 132), one unit alone, and 1026 units at K = 4 and 32 (the grid-stride walk whatever the
    occupancy); some s2 negative; argmax_out given and NULL (same bits of out).
    measured (e32 in brackets): (3, 8, K) 1.9e-7 .. 3.3e-7 (2.1e-7 .. 3.0e-7), worst 3.28e-7 (2.36e-7) at K = 20;
    (2, 132, K) 2.5e-7 .. 3.8e-7 (2.5e-7 .. 3.8e-7), worst 3.81e-7 (3.42e-7) at K = 20; (1, 4, 4) 1.58e-7 (2.09e-7);
    (2, 2052, 4) 3.42e-7 (3.39e-7); (2, 2052, 32) 3.54e-7 (2.69e-7).  No figure is above 1.39 x its e32, and every one of
    the 64 B N winners of every case was the float64 maximum within the bound."""
    B, N, K = case.B, case.N, case.K
    ops = E.make(case)
    ref, ref_am, v, bound = E.reference(**ops)
    e32 = ((E.reference(**ops, dtype=torch.float32)[0].double() - ref).abs().max() / ref.abs().max()).item()
    rc, out, am, untouched = _call(lib, ops, B, N, K)
    assert untouched, "a column beside out or a guard was written"
    rc2, out2, _, untouched2 = _call(lib, ops, B, N, K, want_argmax=False)
    assert untouched2, "without argmax_out: a column beside out, a guard or the argmax buffer was written"
    assert _same_bits(out, out2), "out depends on argmax_out being given"
    assert bool(torch.isfinite(out).all())
    err = ((out.double() - ref).abs().max() / ref.abs().max()).item()
    print("EF| %-14s out err %.2e  e32 %.2e" % (case.name, err, e32))
    assert err <= BAR["out"], err
    assert am.dtype == torch.int32 and int(am.min()) >= 0 and int(am.max()) < K
    ok = E.winners_ok(v, am, bound)
    assert bool(ok.all()), "%d of %d winners are not the float64 maximum within the bound, first at %s" % (
        int((~ok).sum()), ok.numel(), (~ok).nonzero()[0].tolist())
    # the value written is the value of the slot written
    at = torch.gather(v, 1, am.long().unsqueeze(1)).squeeze(1)
    assert ((out.double() - at).abs() <= bound).all()
    # where the float64 winner leads every other neighbour by more than the bound, its LOWEST slot must have won
    clear = E.other_gap(v, ops["idx"], N) > bound
    low = E.lowest_slot_of_winner(v, ops["idx"], N)
    assert torch.equal(am.long()[clear], low[clear]), "a clear winner's lowest slot did not win"
    assert clear.double().mean().item() >= 1.0 - E.NEAR_TIE_CAP


def test_ties_go_to_the_lowest_slot(lib):
    """A list that names one neighbour in several slots produces exactly equal values: the lowest slot wins, as torch.max.
    Every list here names its first neighbour again in slots 3 and K - 1, and its second one in slot 2; asserted exactly
    on the entries where a repeated neighbour is the float64 winner by more than the bound (about 3 in 8 of them)."""
    case = E.EdgeCase("ties", 2, 64, 8, "")
    B, N, K = case.B, case.N, case.K
    ops = E.make(case, seed=5)
    idx = ops["idx"].clone()
    idx[:, :, 3] = idx[:, :, 0]
    idx[:, :, K - 1] = idx[:, :, 0]
    idx[:, :, 2] = idx[:, :, 1]
    ops["idx"] = idx
    ref, ref_am, v, bound = E.reference(**ops)
    assert bool((v[:, 0] == v[:, 3]).all()) and bool((v[:, 0] == v[:, K - 1]).all()) and bool((v[:, 1] == v[:, 2]).all())
    rc, out, am, untouched = _call(lib, ops, B, N, K)
    assert untouched
    assert bool(E.winners_ok(v, am, bound).all())
    clear = E.other_gap(v, idx, N) > bound
    low = E.lowest_slot_of_winner(v, idx, N)
    repeated = clear & (low <= 1)
    assert repeated.double().mean().item() > 0.2, "too few entries are won by a repeated neighbour"
    assert torch.equal(am.long()[repeated], low[repeated]), "a tie did not go to the lowest slot"
    assert torch.equal(am.long()[clear], low[clear])
    assert not bool(((am == 3) | (am == K - 1) | (am == 2))[clear].any())


def test_ids_outside_the_cloud_are_clamped(lib):
    """Ids -1, N, N + 7, 2^31 - 1 and -2^31 in the lists: out and argmax_out are bit for bit those of the call with the ids
    clamped to [0, N - 1] (include/r3d.h: clamped, never dereferenced), in the first and in the last cloud."""
    case = E.EdgeCase("clamp", 3, 16, 8, "")
    B, N, K = case.B, case.N, case.K
    ops = E.make(case, seed=9)
    idx = ops["idx"].clone()
    bad = (-1, N, N + 7, 2 ** 31 - 1, -2 ** 31)
    for b in (0, B - 1):
        for j, value in enumerate(bad):
            idx[b, (3 * j + b) % N, (j + b) % K] = value
            idx[b, N - 1 - j, K - 1] = value
    assert int((idx < 0).sum()) >= 8 and int((idx >= N).sum()) >= 12
    wild, tame = dict(ops, idx=idx), dict(ops, idx=idx.clamp(0, N - 1))
    _, out_w, am_w, ok_w = _call(lib, wild, B, N, K)
    _, out_t, am_t, ok_t = _call(lib, tame, B, N, K)
    assert ok_w and ok_t
    assert bool(torch.isfinite(out_w).all())
    assert _same_bits(out_w, out_t) and torch.equal(am_w, am_t)
    ref, _, v, bound = E.reference(**wild)  # (the reference clamps too)
    assert bool(E.winners_ok(v, am_w, bound).all()) and ((out_w.double() - ref).abs().max() / ref.abs().max()).item() <= BAR["out"]


def test_every_cloud_equals_its_own_call(lib):
    """B = 3 clouds of different content and the same lists: every cloud has the bits of its own B = 1 call."""
    case = E.EdgeCase("clouds", 3, 20, 12, "")
    B, N, K = case.B, case.N, case.K
    ops = E.make(case, seed=11)
    ops["idx"] = ops["idx"][:1].repeat(B, 1, 1).contiguous()
    _, out, am, ok = _call(lib, ops, B, N, K)
    assert ok
    for b in range(B):
        one = dict(ops, PQ=ops["PQ"][b * N:(b + 1) * N].contiguous(), idx=ops["idx"][b:b + 1].contiguous())
        _, o1, a1, ok1 = _call(lib, one, 1, N, K)
        assert ok1 and _same_bits(out[b * N:(b + 1) * N], o1) and torch.equal(am[b * N:(b + 1) * N], a1), b
    assert not _same_bits(out[:N], out[N:2 * N])


def test_refusals_leave_out_untouched(lib):
    """N % 4 != 0, K in 0, 2, 6, 36, ldo < 64 and a NULL pointer: an error code, nothing launched, the poisoned out and
    argmax buffer keep their bits."""
    base = E.EdgeCase("refuse", 2, 8, 8, "")
    ops = E.make(base)
    rs = np.random.RandomState(1)

    def refused(B, N, K, ldo=LDO, null=None, what=""):
        o = dict(ops, PQ=ops["PQ"][:B * N].contiguous(), idx=torch.from_numpy(E.lists(B, N, max(K, 1), rs)))
        rc, _, _, untouched = _call(lib, o, B, N, K, expect_rc0=False, ldo=ldo, null=null)
        assert rc != 0 and untouched, what
        assert len(lib.r3d_last_error_string()) > 0

    refused(2, 6, 8, what="N % 4 != 0")
    for K in (0, 2, 6, 36):
        refused(2, 8, K, what="K = %d" % K)
    refused(2, 8, 8, ldo=63, what="ldo < 64")
    for name in ("PQ", "idx", "W2", "s2", "t2", "out"):
        refused(2, 8, 8, null=name, what="NULL %s" % name)
    rc, out, am, ok = _call(lib, ops, 2, 8, 8)  # and the same operands are taken when nothing is wrong
    assert rc == 0 and ok
