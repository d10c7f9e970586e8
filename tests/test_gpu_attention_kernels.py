"""The attention training kernels (csrc/attention.hip: forward, dK | dV, dQ in fp32 and in bf16 x 3, pack, row-dot, combine
and sum) through the C ABI (r3d_attention_fwd_train_ep_d, r3d_attention_bwd_ep_d) against float64, at the tile edges, on
strided operands inside poisoned memory, with a q_scale, on sharp softmaxes, at the dropout edges and under every key-axis
split -- at all four head widths and in both matrix arithmetics.

Reference: tests/attn_ref.py (held to autograd, the oracle and the golden vectors in tests/test_attn_ref_host.py).

Bars.  out, dq, dk, dv: max |got - ref64| / max |ref64| over the tensor; lse: max |got - ref64| (absolute).  Each case prints
every figure beside ``e32``, the error the SAME dense formula makes in fp32 on the CPU against float64 on that input.  A bar
is 4 x the worst figure measured on the MI355X for that quantity over this module's cases (the kernels are deterministic:
the margin covers other seeds); a bar outside the sharp class is never above CEIL = 1e-4, the bar of the older attention
tests.  The sharp-softmax class (D) has bars of its own: an fp32 score of size s carries about s 2^-24 of absolute error
into the exponent.  The measured figures stand in each test's docstring."""
import contextlib
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_ref as R
from test_gpu_output_dim import _inputs

pytestmark = pytest.mark.gpu

WIDTHS = (32, 64, 96, 128)
CEIL = 1e-4
# quantity -> bar = 4 x the worst figure measured over the module's cases (where: the comment; all figures: the docstrings)
BAR = dict(out=1.1e-5,        # 2.78e-6 (F, split 3, D = 96 N = 65, fp32; e32 2.76e-6)
           lse=3.7e-5,        # 9.34e-6 absolute (F, cost model, D = 128 N = 2048, fp32; e32 7.43e-6)
           dq=1.0e-5,         # 2.49e-6 (A, D = 128 N = 127 p = 0.1, fp32; e32 1.70e-6)
           dk=1.0e-5,         # 2.56e-6 (A, D = 128 N = 127 p = 0, fp32; e32 2.64e-6)
           dv=9.2e-6,         # 2.30e-6 (F, cost model, D = 128 B = 2 N = 129, bf16 x 3; e32 1.51e-6)
           out_sharp=2.6e-5,  # 6.52e-6 (D = 128 N = 160 p = 0.1, fp32; e32 6.49e-6)
           lse_sharp=1.1e-4,  # 2.83e-5 absolute (D = 96 N = 150 p = 0, fp32; e32 2.83e-5)
           dq_sharp=4.4e-5,   # 1.09e-5 (D = 128 N = 160 p = 0, fp32; e32 1.10e-5)
           dk_sharp=4.3e-5,   # 1.08e-5 (D = 128 N = 160 p = 0, fp32; e32 1.11e-5)
           dv_sharp=2.3e-5)   # 5.80e-6 (D = 96 N = 150 p = 0.1, bf16 x 3; e32 2.50e-6)
assert max(v for k, v in BAR.items() if not k.endswith("_sharp")) <= CEIL

POISON = 0x7FC0BEEF  # a quiet NaN of a fixed bit pattern
GUARD = 64


@pytest.fixture(scope="module")
def lib():
    from r3dfsseg_amd import _lib
    return _lib.load()


def _load():
    from r3dfsseg_amd import _lib
    return _lib.load()


def _check(rc):
    from r3dfsseg_amd import _lib
    _lib.check(rc)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def _arith(lib, mode):
    before = lib.r3d_get_matrix_arith()
    _check(lib.r3d_set_matrix_arith(mode))
    try:
        yield
    finally:
        _check(lib.r3d_set_matrix_arith(before))


def _poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device="cuda").view(torch.float32)


def _intact(t):
    """Every element of the fp32 tensor t still holds the poison's bits."""
    return bool((t.view(torch.int32) == POISON).all().item())


def _bufs(lib, B, N, D, group=0):
    """Contiguous out | lse | dqkv | workspace, each with GUARD poisoned elements behind it (the whole buffers start out
    poisoned)."""
    M = B * N
    words = lib.r3d_attention_ws_words_ep_d(B, N, group, D)
    assert words > 0
    flat = SimpleNamespace(out=_poisoned(M * D + GUARD), lse=_poisoned(M + GUARD), dqkv=_poisoned(M * 3 * D + GUARD),
                           ws=_poisoned(words + GUARD))
    return SimpleNamespace(flat=flat, words=words, out=flat.out[:M * D].view(M, D), lse=flat.lse[:M],
                           dqkv=flat.dqkv[:M * 3 * D].view(M, 3 * D), ws=flat.ws)


def _guards_intact(bf):
    f = bf.flat
    return (_intact(f.out[-GUARD:]) and _intact(f.lse[-GUARD:]) and _intact(f.dqkv[-GUARD:])
            and _intact(f.ws[bf.words:]))


def _fwd(lib, qkv, B, N, D, bf, p, seed, sdev=None, group=0, ws=True):
    return lib.r3d_attention_fwd_train_ep_d(_p(qkv), qkv.stride(0), B, N, _p(bf.out), bf.out.stride(0), _p(bf.lse), p, seed,
                                            _p(sdev), group, D, _p(bf.ws) if ws else None, _st())


def _bwd(lib, qkv, B, N, D, dO, bf, p, seed, sdev=None, group=0, q_scale=1.0, dqkv=None, packed=1, ws=True):
    dqkv = bf.dqkv if dqkv is None else dqkv
    return lib.r3d_attention_bwd_ep_d(_p(qkv), qkv.stride(0), B, N, _p(bf.out), bf.out.stride(0), _p(dO), dO.stride(0),
                                      _p(bf.lse), p, seed, _p(sdev), group, D, q_scale, _p(dqkv), dqkv.stride(0),
                                      _p(bf.ws) if ws else None, packed, _st())


def _sdev(value):
    """The device word of a captured graph's seed, holding `value` (mod 2^32)."""
    value &= 0xFFFFFFFF
    return torch.tensor([value - (1 << 32) if value >= (1 << 31) else value], dtype=torch.int32, device="cuda")


def _run(lib, mode, qkv, B, N, D, dO, p=0.0, seed=0, sdev=None, group=0, q_scale=1.0):
    """Forward + backward in arithmetic `mode` (0 fp32, 1 bf16 x 3) on contiguous, poisoned, guarded buffers; the backward
    once on the forward's workspace (packed q | k | v reused) and once cutting them again: bit for bit the same.
    -> (out, lse, dqkv) on the host."""
    with _arith(lib, mode):
        bf = _bufs(lib, B, N, D, group)
        dqkv2 = torch.empty_like(bf.dqkv)
        _check(_fwd(lib, qkv, B, N, D, bf, p, seed, sdev, group))
        _check(_bwd(lib, qkv, B, N, D, dO, bf, p, seed, sdev, group, q_scale, packed=1))
        _check(_bwd(lib, qkv, B, N, D, dO, bf, p, seed, sdev, group, q_scale, dqkv=dqkv2, packed=0))
        torch.cuda.synchronize()
    assert torch.equal(bf.dqkv, dqkv2), "the backward on the forward's packed operands differs from the one that cuts them"
    assert _guards_intact(bf), "a guard behind out, lse, dqkv or the workspace was written"
    return bf.out.cpu(), bf.lse.cpu(), bf.dqkv.cpu()


def _reference(qkv, B, N, D, dO, keep, p, q_scale=1.0):
    """-> (float64, fp32) results of attn_ref.attention, computed once per case and shared by both arithmetics."""
    return (R.attention(qkv, B, N, D, dO, keep, p, q_scale),
            R.attention(qkv, B, N, D, dO, keep, p, q_scale, dtype=torch.float32))


def _errors(got, want, D, zero_scale=None):
    """got = (out, lse, dqkv), want = attn_ref.attention's tuple -> the five figures.  zero_scale: quantity -> the scale that
    stands in for max |want| where the float64 result is identically zero (N = 1, see test_tile_edges)."""
    out, lse, dqkv = got
    wout, wlse, _, wd = want
    errs = dict(lse=(lse.double() - wlse.double()).abs().max().item())
    parts = dict(out=(out, wout), dq=(dqkv[:, :D], wd[:, :D]), dk=(dqkv[:, D:2 * D], wd[:, D:2 * D]),
                 dv=(dqkv[:, 2 * D:], wd[:, 2 * D:]))
    for k, (g, w) in parts.items():
        if zero_scale and k in zero_scale and w.abs().max().item() == 0.0:
            errs[k] = (g.double() - w.double()).abs().max().item() / zero_scale[k]
        else:
            errs[k] = R.rel(g, w)
    return errs


def _hold(case, got, refs, D, suffix="", zero_scale=None):
    """Print the five figures of one run beside e32, then assert every one against its bar."""
    r64, r32 = refs
    assert all(bool(torch.isfinite(t).all()) for t in got), "%s: a result is not finite" % case
    errs = _errors(got, r64, D, zero_scale)
    e32 = _errors((r32[0], r32[1], r32[3]), r64, D, zero_scale)
    for k in ("out", "lse", "dq", "dk", "dv"):
        print("AK| %-40s %-10s err %.2e  e32 %.2e" % (case, k + suffix, errs[k], e32[k]))
    bad = {k: v for k, v in errs.items() if not v <= BAR[k + suffix]}
    assert not bad, (case, bad)
    return errs


# ----------------------------------------------------------------------------------------------------------------------
# A: tile edges
# ----------------------------------------------------------------------------------------------------------------------
EDGE_N = (1, 31, 32, 33, 64, 65, 127, 128, 129, 160)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("D", WIDTHS)
def test_tile_edges(lib, D, p_drop):
    """A.  N on both sides of the 32-key tile, of two tiles (the bf16 x 3 prologue then covers the whole loop), of the
    128-row workgroup, and one row alone; B = 3, so two clouds start at a row other than 0.
    At N = 1 the float64 dq and dk are identically zero (dS = P (dP - <dP, P>) with P = 1) while the kernels subtract the
    row dot <dO, O>, summed by another kernel in another order, from dP: what is left is rounding of terms of size
    max |dP|, so dq is measured against max |dP| max |k| and dk against max |dP| max |q| there.
    measured, worst over N > 1, both p and both arithmetics (e32 in brackets):
      D  32: out 1.1e-6 (1.0e-6)  lse 3.4e-6 (3.4e-6)  dq 1.9e-6 (1.7e-6)  dk 1.9e-6 (1.1e-6)  dv 9.8e-7 (8.3e-7)
      D  64: out 1.6e-6 (1.6e-6)  lse 5.3e-6 (5.3e-6)  dq 1.8e-6 (1.8e-6)  dk 1.8e-6 (1.5e-6)  dv 1.2e-6 (8.7e-7)
      D  96: out 2.0e-6 (2.0e-6)  lse 6.7e-6 (6.7e-6)  dq 2.0e-6 (1.4e-6)  dk 2.1e-6 (1.5e-6)  dv 1.2e-6 (1.0e-6)
      D 128: out 1.9e-6 (1.8e-6)  lse 6.8e-6 (6.8e-6)  dq 2.5e-6 (1.7e-6)  dk 2.6e-6 (2.6e-6)  dv 1.7e-6 (1.1e-6)
    N = 1, worst over the widths: out 2.2e-7, lse 9.5e-7 (1.3e-6), dq 1.1e-6, dk 1.1e-6, dv 2.5e-7.  The dense fp32 formula
    is exact there (e32 = 0 at p = 0: P = 1, out = v), the kernels are within two fp32 ulps: three bf16 pieces carry 24
    bits of v, and dq, dk are the cancellation described above."""
    B, seed = 3, 4321
    for N in EDGE_N:
        qkv, dO = _inputs(B, N, D, 1000 * D + N)
        keep = R.keep_mask(B, N, seed, p_drop) if p_drop > 0 else None
        refs = _reference(qkv, B, N, D, dO, keep, p_drop)
        zero_scale = None
        if N == 1:
            q, k, v = (qkv[:, D * i:D * (i + 1)].double().cpu() for i in range(3))
            dP = ((dO.double().cpu() * v).sum(-1) / (1.0 - float(np.float32(p_drop)))).abs().max().item()
            zero_scale = dict(dq=dP * k.abs().max().item(), dk=dP * q.abs().max().item())
        for mode in (0, 1):
            got = _run(lib, mode, qkv, B, N, D, dO, p_drop, seed)
            _hold("A D=%d N=%d p=%.1f mode=%d" % (D, N, p_drop, mode), got, refs, D, zero_scale=zero_scale)


# ----------------------------------------------------------------------------------------------------------------------
# B: strides and ownership
# ----------------------------------------------------------------------------------------------------------------------
def _strided_run(lib, mode, qkv, B, N, D, dO, p, seed):
    """The production layout: every operand a column slice of a wider matrix, every buffer the op writes poisoned and
    guarded.  Asserts that nothing but the owned slices changed -> (out, lse, dqkv) on the host."""
    M = B * N
    Q = torch.randn(M, 3 * D + 12, device="cuda")
    Q[:, 8:8 + 3 * D] = qkv
    G = torch.randn(M, 128 + D, device="cuda")
    G[:, 64:64 + D] = dO
    words = lib.r3d_attention_ws_words_ep_d(B, N, 0, D)
    O_ = _poisoned(M * (128 + D) + GUARD)
    DQ = _poisoned(M * (3 * D + 7) + GUARD)
    lse = _poisoned(M + GUARD)
    ws = _poisoned(words + GUARD)
    Om, DQm = O_[:M * (128 + D)].view(M, 128 + D), DQ[:M * (3 * D + 7)].view(M, 3 * D + 7)
    bf = SimpleNamespace(out=Om[:, 64:64 + D], lse=lse[:M], dqkv=DQm[:, 3:3 + 3 * D], ws=ws)
    qv, gv = Q[:, 8:8 + 3 * D], G[:, 64:64 + D]
    assert qv.data_ptr() % 16 == 0 and gv.data_ptr() % 16 == 0
    with _arith(lib, mode):
        _check(_fwd(lib, qv, B, N, D, bf, p, seed))
        _check(_bwd(lib, qv, B, N, D, gv, bf, p, seed, packed=1))
        torch.cuda.synchronize()
    assert _intact(O_[M * (128 + D):]) and _intact(DQ[M * (3 * D + 7):]) and _intact(lse[M:]) and _intact(ws[words:])
    assert _intact(Om[:, :64]) and _intact(Om[:, 64 + D:]), "columns beside out were written"
    assert _intact(DQm[:, :3]) and _intact(DQm[:, 3 + 3 * D:]), "columns beside dqkv were written"
    got = bf.out.cpu(), bf.lse.cpu(), bf.dqkv.cpu()
    assert all(bool(torch.isfinite(t).all()) for t in got)
    return got


@pytest.mark.parametrize("D", WIDTHS)
def test_strided_operands_and_ownership(lib, D):
    """B.  N = 129, p = 0.1: qkv at columns [8, 8 + 3 D) of (M, 3 D + 12), out and dO at columns [64, 64 + D) of
    (M, 128 + D) as in production, dqkv at columns [3, 3 + 3 D) of (M, 3 D + 7); out, dqkv, lse and the workspace inside
    NaNs of a fixed bit pattern with 64 more behind each.  Nothing outside the owned slices changes a bit (the guard past
    r3d_attention_ws_words_ep_d words included), every owned element is finite, and the owned values are bit for bit
    those of the contiguous run, which holds against float64.
    measured, worst over the widths: out 1.8e-6 (1.9e-6)  lse 4.9e-6 (3.6e-6)  dq 2.1e-6 (1.2e-6)  dk 2.1e-6 (1.8e-6)
    dv 1.2e-6 (1.2e-6)."""
    B, N, p, seed = 2, 129, 0.1, 77
    qkv, dO = _inputs(B, N, D, 17 * D + N)
    refs = _reference(qkv, B, N, D, dO, R.keep_mask(B, N, seed, p), p)
    for mode in (0, 1):
        got = _strided_run(lib, mode, qkv, B, N, D, dO, p, seed)
        plain = _run(lib, mode, qkv, B, N, D, dO, p, seed)
        for g, w, name in zip(got, plain, ("out", "lse", "dqkv")):
            assert torch.equal(g, w), (name, mode)
        _hold("B D=%d N=%d mode=%d" % (D, N, mode), got, refs, D)


# ----------------------------------------------------------------------------------------------------------------------
# C: q_scale
# ----------------------------------------------------------------------------------------------------------------------
def _q_scale_case(lib, D, tag):
    """The backward with q_scale 1 and with float32(1 / sqrt(D)) on the same forward: dk | dv bit-equal, dq holds the
    reference with that scale."""
    B, N, p, seed = 2, 129, 0.1, 5
    qs = float(np.float32(1.0 / np.sqrt(D)))
    qkv, dO = _inputs(B, N, D, 23 * D + N)
    keep = R.keep_mask(B, N, seed, p)
    ref1, refs = _reference(qkv, B, N, D, dO, keep, p), _reference(qkv, B, N, D, dO, keep, p, qs)
    for mode in (0, 1):
        one = _run(lib, mode, qkv, B, N, D, dO, p, seed)
        got = _run(lib, mode, qkv, B, N, D, dO, p, seed, q_scale=qs)
        assert torch.equal(one[0], got[0]) and torch.equal(one[1], got[1])
        assert torch.equal(one[2][:, D:], got[2][:, D:]), "dk | dv depend on q_scale"
        assert not torch.equal(one[2][:, :D], got[2][:, :D])
        _hold("%s D=%d q_scale=1 mode=%d" % (tag, D, mode), one, ref1, D)
        _hold("%s D=%d q_scale=%.4f mode=%d" % (tag, D, qs, mode), got, refs, D)


@pytest.mark.parametrize("D", WIDTHS)
def test_q_scale(lib, D):
    """C.  Production passes 1 / temperature: dq = q_scale x the gradient of the scaled q, dk | dv untouched (bit for bit).
    (Under a forced split the sum kernel applies the scale: the same case runs in the child of F.)
    measured, worst over the widths: out 1.3e-6 (1.3e-6)  lse 5.8e-6 (4.9e-6)  dq 1.9e-6 (1.9e-6)  dk 1.8e-6 (1.7e-6)
    dv 1.6e-6 (9.3e-7)."""
    _q_scale_case(lib, D, "C")


# ----------------------------------------------------------------------------------------------------------------------
# D: sharp softmax
# ----------------------------------------------------------------------------------------------------------------------
def _sharp_inputs(B, N, D):
    """Scores of |s| up to 60 .. 100 (the _inputs scores, about 4 in spread, times 4); in the last cloud: query 3
    whose dominant key (score 90 against a spread of 20) is key N - 10, in the last key tile; keys 40 and N - 3 exactly
    equal; query 70 with all scores equal (q = 0)."""
    qkv, dO = _inputs(B, N, D, 99 * D + N)
    qkv, dO = qkv.cpu(), dO.cpu()
    qkv[:, :2 * D] *= 2.0
    r = (B - 1) * N
    q3 = qkv[r + 3, :D]
    qkv[r + N - 10, D:2 * D] = q3 * (90.0 / float(q3.double().pow(2).sum()))
    qkv[r + N - 3, D:2 * D] = qkv[r + 40, D:2 * D]
    qkv[r + 70, :D] = 0.0
    return qkv.cuda(), dO.cuda()


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("N", [160, 150])
@pytest.mark.parametrize("D", WIDTHS)
def test_sharp_softmax(lib, D, N, p_drop):
    """D.  B = 2, N = 160 (five full key tiles, the last one alone in the second 128-row block) and 150 (a ragged last
    tile): rows whose softmax is nearly one-hot, a tie between two equal keys, a uniform row.  The backward computes
    exp(s - lse) on scores it recomputes; the bf16 x 3 forward works in the exp2 domain.  Bars of the `_sharp` class.
    measured, worst over N, p and both arithmetics (e32 in brackets):
      D  32: out 3.4e-6 (3.4e-6)  lse 1.4e-5 (1.4e-5)  dq 5.1e-6 (5.5e-6)  dk 4.5e-6 (8.0e-6)  dv 3.2e-6 (2.0e-6)
      D  64: out 5.4e-6 (5.4e-6)  lse 2.5e-5 (2.5e-5)  dq 4.4e-6 (4.3e-6)  dk 3.8e-6 (4.5e-6)  dv 3.1e-6 (1.7e-6)
      D  96: out 4.9e-6 (5.1e-6)  lse 2.8e-5 (2.8e-5)  dq 8.1e-6 (8.2e-6)  dk 8.5e-6 (8.7e-6)  dv 5.8e-6 (2.5e-6)
      D 128: out 6.5e-6 (6.5e-6)  lse 2.5e-5 (2.5e-5)  dq 1.1e-5 (1.1e-5)  dk 1.1e-5 (1.1e-5)  dv 3.7e-6 (2.8e-6)
    (the kernels lose what the dense fp32 formula loses on these inputs.)"""
    B, seed = 2, 31
    qkv, dO = _sharp_inputs(B, N, D)
    s = (qkv[:, :D].double().view(B, N, D) @ qkv[:, D:2 * D].double().view(B, N, D).transpose(1, 2)).cpu()
    assert 60.0 <= s.abs().max().item() <= 100.0, s.abs().max().item()
    assert s[B - 1, 3].argmax().item() == N - 10 and s[B - 1, 3, N - 10] - s[B - 1, 3].topk(2).values[1] > 20
    assert (s[B - 1, 70] == 0).all() and torch.equal(s[B - 1, :, 40], s[B - 1, :, N - 3])
    keep = R.keep_mask(B, N, seed, p_drop) if p_drop > 0 else None
    refs = _reference(qkv, B, N, D, dO, keep, p_drop)
    for mode in (0, 1):
        got = _run(lib, mode, qkv, B, N, D, dO, p_drop, seed)
        _hold("D D=%d N=%d p=%.1f mode=%d" % (D, N, p_drop, mode), got, refs, D, suffix="_sharp")


# ----------------------------------------------------------------------------------------------------------------------
# E: dropout edges and seeds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_rows_that_lose_every_key_and_a_whole_tile(lib, D):
    """E.  p = 0.9 with the seeds proven in tests/test_attn_ref_host.py: query rows with no key kept (out exactly 0 there,
    everything finite), and a row that loses all of keys 32 .. 63 but keeps keys in the tiles on both sides.
    measured, worst over the widths: rows without a key out 1.2e-6 (1.2e-6)  lse 4.3e-6 (4.3e-6)  dq 1.4e-6 (1.5e-6)
    dk 2.0e-6 (2.0e-6)  dv 1.2e-6 (1.3e-6); tile dropped out 9.1e-7 (7.2e-7)  lse 4.1e-6 (4.1e-6)  dq 1.6e-6 (7.5e-7)
    dk 1.3e-6 (1.1e-6)  dv 1.1e-6 (8.6e-7)."""
    seed, p, B, N = R.ALL_DROPPED
    qkv, dO = _inputs(B, N, D, 3 * D + N)
    refs = _reference(qkv, B, N, D, dO, R.keep_mask(B, N, seed, p), p)
    rows = [b * N + q for b, q in R.ALL_DROPPED_ROWS]
    assert (refs[0][0][rows] == 0).all()
    for mode in (0, 1):
        got = _run(lib, mode, qkv, B, N, D, dO, p, seed)
        assert (got[0][rows] == 0).all(), "out of a row whose every key is dropped is not exactly 0"
        assert int((got[0] == 0).all(1).sum()) == len(rows)
        _hold("E all-dropped D=%d mode=%d" % (D, mode), got, refs, D)
    seed, p, B, N = R.TILE_DROPPED
    qkv, dO = _inputs(B, N, D, 5 * D + N)
    refs = _reference(qkv, B, N, D, dO, R.keep_mask(B, N, seed, p), p)
    for mode in (0, 1):
        got = _run(lib, mode, qkv, B, N, D, dO, p, seed)
        _hold("E tile-dropped D=%d mode=%d" % (D, mode), got, refs, D)


@pytest.mark.parametrize("D", WIDTHS)
def test_seed_identities(lib, D):
    """E.  Bit for bit, forward and backward: (seed = a, *seed_dev = b) is (seed = a + b mod 2^32, NULL) with a + b wrapping;
    with seed_group = g and B = 3 g, clouds [e g, (e + 1) g) are a call on those clouds alone with seed + 2 e (wrapping).
    The batch in groups against float64, measured, worst over the widths: out 1.3e-6 (1.7e-6)  lse 8.8e-6 (5.4e-6)
    dq 1.1e-6 (1.5e-6)  dk 1.9e-6 (1.8e-6)  dv 9.6e-7 (1.1e-6)."""
    p, N = 0.1, 65
    a, b = 0xFFFFFFF0, 0x25
    qkv, dO = _inputs(2, N, D, 7 * D)
    g, seed = 2, 0xFFFFFFFF
    qkv6, dO6 = _inputs(3 * g, N, D, 9 * D)
    for mode in (0, 1):
        x = _run(lib, mode, qkv, 2, N, D, dO, p, a, sdev=_sdev(b))
        y = _run(lib, mode, qkv, 2, N, D, dO, p, (a + b) & 0xFFFFFFFF)
        z = _run(lib, mode, qkv, 2, N, D, dO, p, a)
        assert all(torch.equal(s, t) for s, t in zip(x, y)), mode
        assert not torch.equal(x[0], z[0]) and not torch.equal(x[2], z[2])  # the device word counts
        whole = _run(lib, mode, qkv6, 3 * g, N, D, dO6, p, seed, group=g)
        for e in range(3):
            rows = slice(e * g * N, (e + 1) * g * N)
            alone = _run(lib, mode, qkv6[rows], g, N, D, dO6[rows], p, (seed + 2 * e) & 0xFFFFFFFF)
            assert all(torch.equal(s[rows], t) for s, t in zip(whole, alone)), (mode, e)
    keep = R.keep_mask(3 * g, N, seed, p, group=g)
    _hold("E groups D=%d mode=1" % D, whole, _reference(qkv6, 3 * g, N, D, dO6, keep, p), D)


def test_the_kernels_mask_in_groups():
    """E.  Width 64, N = 65, seed_group = 2, a wrapping seed and a device word: with v = identity columns and q = k = 0 the
    output IS the dropped attention matrix on the first 64 keys (two key tiles), so the kernels' own mask is read off and
    compared with attn_ref.keep_mask; the backward's mask through dv = P~^T dO with dO = identity columns."""
    lib = _load()
    D, N, g, p, seed, dev = 64, 65, 2, 0.1, 0xFFFFFFFE, 5
    B = 2 * g
    qkv = torch.zeros(B * N, 3 * D)
    qkv[:, 2 * D:] = torch.eye(N, D).repeat(B, 1)
    qkv = qkv.cuda()
    dO = torch.eye(N, D).repeat(B, 1).cuda()  # dO[query] = e_query: dv[key][c] = P~[query c][key]
    want = R.keep_mask(B, N, seed, p, seed_dev=dev, group=g)
    assert not torch.equal(want[:g], want[g:])
    for mode in (0, 1):
        out, _, dqkv = _run(lib, mode, qkv, B, N, D, dO, p, seed, sdev=_sdev(dev), group=g)
        assert torch.equal(out.view(B, N, D) > 0, want[..., :D]), mode
        dv = dqkv[:, 2 * D:].view(B, N, D)  # [b][key][query < 64]
        assert torch.equal(dv.transpose(1, 2) > 0, want[:, :D, :]), mode


# ----------------------------------------------------------------------------------------------------------------------
# F: key-axis splits (R3D_ATT_SPLIT is read once per process: child processes)
# ----------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import test_gpu_attention_kernels as T
T.%(fn)s()
print("CHILD_OK")
"""


def _child(fn, split):
    here = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD % {"root": os.path.dirname(here), "tests": here, "fn": fn}
    env = dict(os.environ, R3D_ATT_SPLIT=split)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def _child_forced_split():
    lib = _load()
    assert os.environ["R3D_ATT_SPLIT"] == "3"
    p, seed, B = 0.1, 11, 2
    for D in WIDTHS:
        for N in (33, 65, 129, 500):  # 2 tiles: the split clipped to 2; 3 tiles: one per range; 5 = 2 + 2 + 1; 16 = 6 + 6 + 4
            qkv, dO = _inputs(B, N, D, 31 * D + N)
            refs = _reference(qkv, B, N, D, dO, R.keep_mask(B, N, seed, p), p)
            for mode in (0, 1):
                _hold("F split=3 D=%d N=%d mode=%d" % (D, N, mode), _run(lib, mode, qkv, B, N, D, dO, p, seed), refs, D)
        _q_scale_case(lib, D, "F split=3")


def _child_cost_model():
    lib = _load()
    assert os.environ["R3D_ATT_SPLIT"] == "0"
    p, seed = 0.1, 0xFFFFFFFF
    for D in (64, 128):
        for g, N in ((1, 512), (2, 129), (1, 2048)):
            B = 3 * g
            qkv, dO = _inputs(B, N, D, 37 * D + N)
            one = slice(0, g * N)
            refs = _reference(qkv[one], g, N, D, dO[one], R.keep_mask(g, N, seed, p), p)  # once, for both arithmetics
            for mode in (0, 1):
                alone = _run(lib, mode, qkv[one], g, N, D, dO[one], p, seed)
                _hold("F split=0 D=%d B=%d N=%d mode=%d" % (D, g, N, mode), alone, refs, D)
                whole = _run(lib, mode, qkv, B, N, D, dO, p, seed, group=g)  # the split is chosen per episode
                for e in range(3):
                    rows = slice(e * g * N, (e + 1) * g * N)
                    if e:
                        alone = _run(lib, mode, qkv[rows], g, N, D, dO[rows], p, (seed + 2 * e) & 0xFFFFFFFF)
                    assert all(torch.equal(s[rows], t) for s, t in zip(whole, alone)), (D, g, N, mode, e)


def test_forced_split():
    """F.  R3D_ATT_SPLIT=3 at every width, N = 33 (two tiles: the split is clipped), 65 (one tile per range), 129 and 500
    (ragged last range), p = 0.1, both arithmetics: all five quantities against float64, the workspace guard intact, and
    the q_scale case of C (the sum kernel applies the scale to the dQ partials).
    measured, worst over N and both arithmetics (e32 in brackets):
      D  32: out 1.2e-6 (1.1e-6)  lse 3.7e-6 (3.7e-6)  dq 1.4e-6 (8.1e-7)  dk 1.3e-6 (1.4e-6)  dv 9.9e-7 (5.4e-7)
      D  64: out 1.4e-6 (1.4e-6)  lse 5.2e-6 (5.2e-6)  dq 1.6e-6 (1.7e-6)  dk 1.3e-6 (1.7e-6)  dv 1.1e-6 (8.5e-7)
      D  96: out 2.8e-6 (2.8e-6)  lse 5.8e-6 (5.8e-6)  dq 1.8e-6 (1.9e-6)  dk 1.9e-6 (2.8e-6)  dv 1.9e-6 (2.1e-6)
      D 128: out 1.8e-6 (1.2e-6)  lse 8.4e-6 (8.4e-6)  dq 1.6e-6 (1.7e-6)  dk 2.0e-6 (1.8e-6)  dv 1.7e-6 (8.0e-7)"""
    _child("_child_forced_split", "3")


def test_cost_model_split():
    """F.  R3D_ATT_SPLIT=0, the cost model that also sizes the workspace, at D = 64 and 128 on (B, N) = (1, 512), (2, 129),
    (1, 2048): all five quantities against float64, the workspace guard intact, and a batch of 3 g clouds with
    seed_group = g bit for bit the three g-cloud calls.
    measured, worst over the shapes and both arithmetics (e32 in brackets):
      D  64: out 1.4e-6 (1.4e-6)  lse 5.9e-6 (5.9e-6)  dq 1.8e-6 (2.0e-6)  dk 1.5e-6 (1.2e-6)  dv 1.5e-6 (1.4e-6)
      D 128: out 2.0e-6 (1.7e-6)  lse 9.3e-6 (7.4e-6)  dq 2.2e-6 (2.2e-6)  dk 2.3e-6 (1.6e-6)  dv 2.3e-6 (1.5e-6)"""
    _child("_child_cost_model", "0")


# ----------------------------------------------------------------------------------------------------------------------
# G: no workspace
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_without_a_workspace(lib, D):
    """G.  The forward with ws = NULL in bf16 x 3 mode takes the fp32 kernel: bit for bit the mode-0 call with a workspace
    (no split by default).  The backward with ws = NULL is refused before any launch: dqkv keeps its poison."""
    B, N, p, seed = 2, 129, 0.1, 3
    qkv, dO = _inputs(B, N, D, 41 * D)
    with _arith(lib, 0):
        a = _bufs(lib, B, N, D)
        _check(_fwd(lib, qkv, B, N, D, a, p, seed))
    with _arith(lib, 1):
        b = _bufs(lib, B, N, D)
        _check(_fwd(lib, qkv, B, N, D, b, p, seed, ws=False))
        torch.cuda.synchronize()
        assert torch.equal(a.out, b.out) and torch.equal(a.lse, b.lse)
        assert _intact(b.flat.ws) and _guards_intact(b) and _guards_intact(a)
        assert _bwd(lib, qkv, B, N, D, dO, b, p, seed, ws=False) != 0
        assert "null pointer" in lib.r3d_last_error_string().decode()
        torch.cuda.synchronize()
        assert _intact(b.flat.dqkv) and _intact(b.flat.ws)
