"""The GEMM family that decides no index, kernel by kernel through the C ABI against float64, at every tile edge, in both
matrix arithmetics and inside poisoned memory:

  r3d_pointwise_gemm_kernel (csrc/gemm.hip), r3d_pointwise_gemm_bx3_kernel, r3d_w_pack_bx3_kernel +
  r3d_pointwise_gemm_bx3p_kernel (csrc/gemm_bx3.hip) behind r3d_pointwise_conv / _acc / _stats;
  r3d_gemm_tn_kernel (csrc/train_ops.hip), r3d_gemm_tn_bx3_kernel (csrc/gemm_bx3.hip) + r3d_chunk_reduce_kernel behind
  r3d_gemm_tn.

Cases and the kernel each one claims: tests/gemm_cases.py (held to r3d_debug_pointwise_path / r3d_debug_gemm_tn_plan in
tests/test_gemm_ref_host.py; every run here asserts the path again, from the pointers it really passes).  Reference:
tests/gemm_ref.py.

Layout.  X is a column slice of a wider matrix, Out a column slice of another, W sits between guards, A and B are slices of
wider matrices with odd row pitches; everything around the operands holds POISON, a quiet NaN of a fixed bit pattern, and
has to hold it after every call: the padding columns, the rows beyond M, the guards, the tail of every workspace.  A kernel
that reads one element it does not own returns a NaN, one that writes one is caught by the bits.

Figures.  Point-wise: max |got - ref64| / (|scale| sum_k |x||w| + |shift| [+ |pre| when accumulating]); gemm_tn:
max |got - ref64| / (|alpha| sum_m |a||b| [+ |pre|]).  Each case prints its figure beside ``e32``, the figure of the same
sum in fp32 as one running sum on the CPU.  A bar is 4 x the worst figure measured on the MI355X over this module's cases
(the kernels are deterministic: the margin covers other seeds) and never above CEIL = 4e-7, the bar of the older
``*_both_arithmetics`` tests.  The measured figures stand in each test's docstring."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import gemm_cases as C
import gemm_ref as R

pytestmark = pytest.mark.gpu

CEIL = 4e-7
# quantity -> bar = 4 x the worst figure measured over the module's cases (where: the comment; all figures: the docstrings)
# 4 x either worst figure is above CEIL, so CEIL is the bar of both quantities: the margin left is 1.18 (pw) and 1.43 (tn)
BAR = dict(pw=min(4 * 3.38e-7, CEIL),   # 3.38e-7 (A, (256, 96, 132) plain, fp32 kernel under arithmetic 0; e32 2.52e-7)
           tn=min(4 * 2.80e-7, CEIL))   # 2.80e-7 (E, (1, 257, 33), bf16 x 3; e32 5.88e-8 -- see test_gemm_tn_tile_and_chunk_edges)
assert max(BAR.values()) <= CEIL

POISON = 0x7FC0BEEF  # a quiet NaN of a fixed bit pattern
GUARD = 64           # floats (256 bytes: a guard in front keeps the 16-byte alignment of what follows)
EXTRA = 3            # poisoned rows behind the M rows of every row-major operand
MASK0 = int(os.environ.get("R3D_GEMM_BX3", 7))  # the r3d_debug_set_gemm_bx3 mask of the process (r3dfsseg_amd/_lib.py)


@pytest.fixture(scope="module")
def lib():
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
def _setting(lib, arith, mask):
    """r3d_set_matrix_arith(arith) and r3d_debug_set_gemm_bx3(mask) for the block.  The mask has no getter: afterwards it is
    what the process started with (_lib.load: R3D_GEMM_BX3, else all three bits)."""
    a0 = lib.r3d_get_matrix_arith()
    _check(lib.r3d_set_matrix_arith(arith))
    _check(lib.r3d_debug_set_gemm_bx3(mask))
    try:
        yield
    finally:
        _check(lib.r3d_debug_set_gemm_bx3(MASK0))
        _check(lib.r3d_set_matrix_arith(a0))


class Slab:
    """A poisoned flat buffer GUARD | rows x ld | GUARD whose columns [c0, c0 + C) of the first M rows are the operand."""

    def __init__(self, M, C, ld, c0, data=None, rows=None, off=0):
        rows = M + EXTRA if rows is None else rows
        self.M, self.C, self.ld, self.c0, self.rows, self.off = M, C, ld, c0, rows, off
        self.flat = torch.full((GUARD + off + rows * ld + GUARD,), POISON, dtype=torch.int32, device="cuda").view(torch.float32)
        self.wide = self.flat[GUARD + off:GUARD + off + rows * ld].view(rows, ld)
        self.view = self.wide[:M, c0:c0 + C]
        if data is not None:
            self.view.copy_(torch.as_tensor(data).to("cuda"))

    def rest_intact(self):
        """Everything but the operand itself still holds the poison's bits."""
        bits = self.flat.view(torch.int32).clone()
        bits[GUARD + self.off:GUARD + self.off + self.rows * self.ld].view(self.rows, self.ld)[:self.M, self.c0:self.c0 + self.C] = POISON
        return bool((bits == POISON).all().item())

    def bits(self):
        return self.view.contiguous().view(torch.int32).cpu()

    def host(self):
        return self.view.cpu()


def _vec(data, off=0):
    """A contiguous operand (W, scale, shift, a workspace) between two poisoned guards, `off` floats behind 16-byte alignment."""
    data = torch.as_tensor(data)
    return Slab(1, data.numel(), data.numel(), 0, data.reshape(1, -1), rows=1, off=off)


def _rs(seed):
    return np.random.RandomState(seed)


@functools.lru_cache(maxsize=None)
def _pw_inputs(M, K, Co, seed=0):
    """-> X, W, scale, shift, pre (numpy fp32): a row of X 1e4 times the others (a wide dynamic range inside one output
    column), some scales negative and one exactly 0."""
    r = _rs(1000003 * M + 1009 * K + Co + seed)
    X = r.randn(M, K).astype(np.float32)
    X[5 % M] *= 1e4
    W = (r.randn(Co, K) / np.sqrt(K)).astype(np.float32)
    scale = (r.randn(Co) * 0.3 + 1.0).astype(np.float32)
    scale[::3] *= -1.0
    if Co > 1:
        scale[1] = 0.0
    shift = (r.randn(Co) * 0.3).astype(np.float32)
    pre = r.randn(M, Co).astype(np.float32)
    return X, W, scale, shift, pre


@functools.lru_cache(maxsize=None)
def _pw_refs(M, K, Co, sc, sh, act, acc, seed=0):
    """-> (ref64, bound, e32) of one point-wise call: computed once, shared by both arithmetics and every kernel."""
    X, W, scale, shift, pre = _pw_inputs(M, K, Co, seed)
    args = (X, W, scale if sc else None, shift if sh else None)
    ref = R.pointwise(*args, act, pre if acc else None)
    bound = R.pointwise_bound(*args, pre if acc else None)
    return ref, bound, R.figure(R.pointwise32(*args, act, pre if acc else None), ref, bound)


def _pw_call(lib, M, K, Co, sc=0, sh=0, act=0, acc=0, path=None, geometry=None, w_off=0, stats=False, seed=0):
    """One call of r3d_pointwise_conv (acc: _acc; stats: _stats) on poisoned slabs under the current setting.  Asserts the
    path the launcher takes for these pointers (when `path` is given), the return code and that nothing but Out's slice
    (and the statistics) was written.  -> Out's slice on the host (stats: and the 2 Co sums)."""
    Xn, Wn, scn, shn, pren = _pw_inputs(M, K, Co, seed)
    ldx, x0, ldo, o0 = geometry or (K + 8, 4, Co + 8 + (-Co) % 4, 4)
    X, W = Slab(M, K, ldx, x0, Xn), _vec(Wn, w_off)
    S, T = (_vec(scn) if sc else None), (_vec(shn) if sh else None)
    O_ = Slab(M, Co, ldo, o0, pren if acc else None)
    xv, wv, ov = X.view, W.view, O_.view
    if path is not None:
        got = lib.r3d_debug_pointwise_path(M, K, Co, ldx, ldo, xv.data_ptr() % 16, wv.data_ptr() % 16, ov.data_ptr() % 16, 0)
        assert got == path, "path %d, the case claims %d" % (got, path)
    x_before = X.flat.view(torch.int32).clone()
    if stats:
        words = lib.r3d_pointwise_conv_stats_ws_words(M, Co)
        ws, sums = Slab(1, words, words, 0, rows=1), Slab(1, 2 * Co, 2 * Co, 0, rows=1)
        _check(lib.r3d_pointwise_conv_stats(_p(xv), ldx, _p(wv), M, K, Co, _p(ov), ldo, _p(sums.view), _p(ws.view), _st()))
    else:
        fn = lib.r3d_pointwise_conv_acc if acc else lib.r3d_pointwise_conv
        _check(fn(_p(xv), ldx, _p(wv), M, K, Co, _p(S.view) if S else None, _p(T.view) if T else None, act, _p(ov), ldo, _st()))
    torch.cuda.synchronize()
    assert O_.rest_intact(), "Out: a padding column, a row beyond M or a guard was written"
    assert torch.equal(X.flat.view(torch.int32), x_before) and W.rest_intact(), "X or W changed"
    assert (S is None or S.rest_intact()) and (T is None or T.rest_intact())
    if stats:
        assert ws.rest_intact() and sums.rest_intact(), "the workspace's tail or the guard behind the sums was written"
        return O_.host(), sums.host().reshape(2, Co)
    return O_.host()


def _pw_hold(case, got, M, K, Co, sc, sh, act, acc, seed=0):
    ref, bound, e32 = _pw_refs(M, K, Co, sc, sh, act, acc, seed)
    err = R.figure(got.numpy(), ref, bound)
    print("GK| %-44s pw err %.2e  e32 %.2e" % (case, err, e32))
    assert err <= BAR["pw"], (case, err)
    return err


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# A: every tile edge of every kernel
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("kernel", ["fp32", "bx3", "bx3p"])
def test_pointwise_tile_edges(lib, kernel, arith):
    """A.  gemm_cases.SWEEPS: one axis sweeps, the others sit at an edge value; each shape PLAIN (no scale, shift,
    activation) and with all three (LeakyReLU).  Under arithmetic 0 every shape runs on the fp32 kernel.  Under arithmetic 1
    every shape with M >= 256 runs on both bf16 kernels (masks 3 and 7), which give the same bits.
    measured, worst per group of shapes (e32 of that case in brackets):
      fp32 shapes: 2.26e-7 (2.26e-7) under either arithmetic, (129, 33, 65)
      bx3 shapes:  arithmetic 0 3.38e-7 (2.52e-7) at (256, 96, 132); arithmetic 1 2.65e-7 (2.27e-7) at (129, 160, 132) LeakyReLU
      bx3p shapes: arithmetic 0 3.38e-7 (2.52e-7) at (256, 96, 132); arithmetic 1 3.24e-7 (2.72e-7) at (383, 96, 132)
    No figure of the module's point-wise cases is above 1.52 x its e32."""
    worst = 0.0
    for c in (c for c in C.SWEEPS if c.name.startswith(kernel + " ")):
        for sc, sh, act in ((0, 0, 0), (1, 1, 2)):
            tag = "A %s%s arith %d" % (c.name, " lrelu" if act else "", arith)
            with _setting(lib, arith, c.mask):
                got = _pw_call(lib, c.M, c.K, c.Co, sc, sh, act, path=c.path if arith else 0, geometry=C.pw_geometry(c))
            worst = max(worst, _pw_hold(tag, got, c.M, c.K, c.Co, sc, sh, act, 0))
            if arith and c.path and c.M >= 256:
                with _setting(lib, 1, c.mask ^ 4):
                    other = _pw_call(lib, c.M, c.K, c.Co, sc, sh, act, path=3 - c.path, geometry=C.pw_geometry(c))
                assert _same_bits(got, other), "%s: the two bf16 kernels differ" % tag
    print("GK| worst A %s arith %d: %.2e" % (kernel, arith, worst))


def test_packed_scratch_is_reused_and_grows(lib):
    """A.  The packed-W scratch of a stream: made by the stream's first call, reused by the second (same bits), replaced by a
    larger one when Co K outgrows it (launches already queued keep the old one), and reused again by a small call after."""
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), _setting(lib, 1, 7):
        outs = []
        for c in (C.GROW_SMALL, C.GROW_SMALL, C.GROW_LARGE, C.GROW_SMALL, C.GROW_LARGE):
            got = _pw_call(lib, c.M, c.K, c.Co, 1, 1, 2, path=2, geometry=C.pw_geometry(c))
            _pw_hold("A %s" % c.name, got, c.M, c.K, c.Co, 1, 1, 2, 0)
            outs.append(got)
        assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[3]) and _same_bits(outs[2], outs[4])
        with _setting(lib, 1, 3):
            other = _pw_call(lib, C.GROW_LARGE.M, C.GROW_LARGE.K, C.GROW_LARGE.Co, 1, 1, 2, path=1, geometry=C.pw_geometry(C.GROW_LARGE))
        assert _same_bits(outs[2], other)


# ----------------------------------------------------------------------------------------------------------------------
# B: the epilogue, crossed with the kernels
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("case", C.EPILOGUE, ids=[c.name.replace(" ", "-") for c in C.EPILOGUE])
def test_pointwise_epilogue(lib, case, arith):
    """B.  act 0, 1, 2 x (scale, shift) given or NULL x accumulate 0, 1 (into a pre-filled Out) on one full-tile and one tail
    shape per kernel; some scales negative, one exactly 0 (its column is act(shift), or 0 exactly without a shift).
    r3d_pointwise_conv_stats on the same shape: Out has the bits of the plain call, the column sums are those of Out.
    The packed kernel's six (PLAIN, STATS, FULL) variants all run here, the four without STATS with accumulate too
    (tests/test_gemm_ref_host.py derives that from the shapes).  For M >= 256 both bf16 kernels give the same bits.
    measured, worst over the cross (e32 in brackets): arithmetic 0 2.95e-7 (2.95e-7), (281, 96, 132) act 0 with scale and
    shift; arithmetic 1 2.17e-7 (1.68e-7), (64, 32, 64) act 0 with scale (mask 0: the fp32 kernel)."""
    c = case
    path = c.path if arith else 0
    geo = C.pw_geometry(c)
    worst, plain = 0.0, None
    for act in C.ACTS:
        for sc, sh in C.AFFINE:
            for acc in (0, 1):
                tag = "B %s act %d sc %d sh %d acc %d arith %d" % (c.name, act, sc, sh, acc, arith)
                with _setting(lib, arith, c.mask):
                    got = _pw_call(lib, c.M, c.K, c.Co, sc, sh, act, acc, path=path, geometry=geo)
                worst = max(worst, _pw_hold(tag, got, c.M, c.K, c.Co, sc, sh, act, acc))
                if (act, sc, sh, acc) == (0, 0, 0, 0):
                    plain = got
                if arith and path and c.M >= 256:
                    with _setting(lib, 1, c.mask ^ 4):
                        other = _pw_call(lib, c.M, c.K, c.Co, sc, sh, act, acc, path=3 - path, geometry=geo)
                    assert _same_bits(got, other), "%s: the two bf16 kernels differ" % tag
    with _setting(lib, arith, c.mask):
        raw, sums = _pw_call(lib, c.M, c.K, c.Co, path=path, geometry=geo, stats=True)
    assert _same_bits(raw, plain), "r3d_pointwise_conv_stats writes another Out than r3d_pointwise_conv"
    r64 = raw.double().numpy()
    np.testing.assert_allclose(sums[0].numpy(), r64.sum(0), rtol=1e-5, atol=2e-6 * np.abs(r64).sum(0).max())
    np.testing.assert_allclose(sums[1].numpy(), (r64 * r64).sum(0), rtol=1e-5)
    if arith and path and c.M >= 256:
        with _setting(lib, 1, c.mask ^ 4):
            raw2, sums2 = _pw_call(lib, c.M, c.K, c.Co, path=3 - path, geometry=geo, stats=True)
        assert _same_bits(raw, raw2) and _same_bits(sums, sums2), "statistics: the two bf16 kernels differ"
    print("GK| worst B %s arith %d: %.2e" % (c.name, arith, worst))


# ----------------------------------------------------------------------------------------------------------------------
# C: fall-backs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.FALLBACKS, ids=[c.name for c in C.FALLBACKS])
def test_pointwise_fallbacks(lib, case):
    """C.  Under arithmetic 1 and the default mask, each shape breaks one rule of the bf16 forms: the path function says
    fp32 for the pointers really passed (a view 1 float into a 16-byte aligned buffer is 4 bytes off), the result meets the
    same bar and the padding is intact.  measured, worst: 2.08e-7 (e32 1.66e-7) at Co = 28."""
    c = case
    geo = C.fb_geometry(c)
    with _setting(lib, 1, 7):
        base = lib.r3d_debug_pointwise_path(256, 64, 64, 72, 72, 0, 0, 0, 0)
        got = _pw_call(lib, c.M, c.K, c.Co, 1, 1, 2, path=0, geometry=geo, w_off=c.w_off)
        acc = _pw_call(lib, c.M, c.K, c.Co, 1, 1, 2, 1, path=0, geometry=geo, w_off=c.w_off)
    assert base == 2
    _pw_hold("C %s (%s)" % (c.name, c.rule), got, c.M, c.K, c.Co, 1, 1, 2, 0)
    _pw_hold("C %s (%s) acc" % (c.name, c.rule), acc, c.M, c.K, c.Co, 1, 1, 2, 1)


# ----------------------------------------------------------------------------------------------------------------------
# D: a row is a function of its own row
# ----------------------------------------------------------------------------------------------------------------------
ROWS = [("fp32", 0, 7, 0), ("bx3", 1, 3, 1), ("bx3p", 1, 7, 2)]


@pytest.mark.parametrize("name,arith,mask,path", ROWS, ids=[r[0] for r in ROWS])
def test_a_row_is_a_function_of_its_own_row(lib, name, arith, mask, path):
    """D.  M = 700 rows, K = 64, Co = 68.  (1) The call on rows [37, 37 + 300) of the same X (37 is a multiple of no tile
    height; both calls stay inside one kernel) gives the bits those rows have in the whole call.  (2) With row 5 of X set
    to inf and row 77 to NaN every other row keeps its bits, and those two rows are not finite anywhere."""
    M, K, Co, r0, M1 = 700, 64, 68, 37, 300
    Xn, Wn, _, _, _ = _pw_inputs(M, K, Co)
    ldx, ldo = K + 8, Co + 8

    def run(Xdata):
        m = Xdata.shape[0]
        X, W, O_ = Slab(m, K, ldx, 4, Xdata), _vec(Wn), Slab(m, Co, ldo, 4)
        with _setting(lib, arith, mask):
            assert lib.r3d_debug_pointwise_path(m, K, Co, ldx, ldo, X.view.data_ptr() % 16, W.view.data_ptr() % 16,
                                                O_.view.data_ptr() % 16, 0) == path
            _check(lib.r3d_pointwise_conv(_p(X.view), ldx, _p(W.view), m, K, Co, None, None, 0, _p(O_.view), ldo, _st()))
        torch.cuda.synchronize()
        assert O_.rest_intact()
        return O_.host()

    whole = run(Xn)
    assert bool(torch.isfinite(whole).all())
    assert _same_bits(run(Xn[r0:r0 + M1]), whole[r0:r0 + M1]), "rows [37, 337) alone differ from the same rows of the whole call"
    Xbad = Xn.copy()
    Xbad[5], Xbad[77] = np.inf, np.nan
    bad = run(Xbad)
    keep = torch.ones(M, dtype=torch.bool)
    keep[[5, 77]] = False
    assert _same_bits(bad[keep], whole[keep]), "an inf or NaN row of X reached another row of Out"
    assert not bool(torch.isfinite(bad[[5, 77]]).any()), "a row of inf / NaN inputs has a finite output"


# ----------------------------------------------------------------------------------------------------------------------
# E: r3d_gemm_tn
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tn_inputs(M, Ca, Cb):
    r = _rs(7919 * M + 131 * Ca + Cb)
    A = r.randn(M, Ca).astype(np.float32)
    # a COLUMN of A 1e4 times the others: a wide dynamic range between outputs.  (Not a row: one term 1e4 times the others
    # in every sum costs any fp32 summation ~sqrt(M) ulps of THAT term, 8.4e-7 of the bound at M = 70 for the fp32 running
    # sum on the CPU and for the fp32 kernel alike -- an input property, not a kernel's.)
    A[:, 5 % Ca] *= 1e4
    return A, r.randn(M, Cb).astype(np.float32), r.randn(Ca, Cb).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _tn_refs(M, Ca, Cb, alpha, acc):
    A, B, pre = _tn_inputs(M, Ca, Cb)
    ref = R.gemm_tn(A, B, alpha, pre if acc else None)
    bound = R.gemm_tn_bound(A, B, alpha, pre if acc else None)
    return ref, bound, R.figure(R.gemm_tn32(A, B, alpha, pre if acc else None), ref, bound)


def _odd(n):
    return n | 1


def _tn_call(lib, c, arith, alpha=1.0, acc=0):
    """r3d_gemm_tn twice on slices of wider poisoned matrices with odd row pitches, into a guarded out and a workspace of
    exactly r3d_gemm_tn_ws_words floats with a guard; asserts the plan, the same bits from both calls, and the poison."""
    An, Bn, pren = _tn_inputs(c.M, c.Ca, c.Cb)
    lda, ldb = _odd(c.Ca + 9), _odd(c.Cb + 5)
    A, B = Slab(c.M, c.Ca, lda, 3, An), Slab(c.M, c.Cb, ldb, 2, Bn)
    outs = []
    with _setting(lib, arith, 7):
        rows, chunks = ctypes.c_int(-1), ctypes.c_int(-1)
        plan = lib.r3d_debug_gemm_tn_plan(c.M, c.Ca, c.Cb, ctypes.byref(rows), ctypes.byref(chunks))
        assert (plan, rows.value, chunks.value) == (c.plan if arith else 0, c.rows, c.chunks), (plan, rows.value, chunks.value)
        words = lib.r3d_gemm_tn_ws_words(c.M, c.Ca, c.Cb)  # (the same under either arithmetic)
        assert words >= chunks.value * c.Ca * c.Cb
        for _ in range(2):
            out = Slab(c.Ca, c.Cb, c.Cb, 0, pren if acc else None, rows=c.Ca)
            ws = Slab(1, words, words, 0, rows=1)
            _check(lib.r3d_gemm_tn(_p(A.view), lda, _p(B.view), ldb, c.M, c.Ca, c.Cb, alpha, _p(out.view), acc, _p(ws.view), _st()))
            torch.cuda.synchronize()
            assert out.rest_intact() and ws.rest_intact(), "a guard behind out or behind the workspace was written"
            outs.append(out.host())
    assert A.rest_intact() and B.rest_intact()
    assert _same_bits(outs[0], outs[1]), "two calls differ"
    return outs[0]


def _tn_hold(case, got, c, alpha, acc):
    ref, bound, e32 = _tn_refs(c.M, c.Ca, c.Cb, alpha, acc)
    err = R.figure(got.numpy(), ref, bound)
    print("GK| %-44s tn err %.2e  e32 %.2e" % (case, err, e32))
    assert err <= BAR["tn"], (case, err)
    return err


@pytest.mark.parametrize("arith", [0, 1])
def test_gemm_tn_tile_and_chunk_edges(lib, arith):
    """E.  gemm_cases.TN_CASES: a last chunk of 1, 31, 32, 33 rows (and M = 1, 70, 127, 128) under 128 x 128 and under
    256 x 64 tiles, Ca and Cb on both sides of every tile, the fp32 fall-backs (Cb = 9 among them); the rows behind M and
    the columns beside A and B are NaN.
    measured, worst (e32 in brackets): arithmetic 0 2.50e-7 (3.04e-7) at (129, 257, 33); arithmetic 1 2.80e-7 (5.88e-8) at
    (1, 257, 33) and 2.67e-7 (5.83e-8) at (1, 33, 65).  Those two are the only figures of the module above 4 x e32, and they
    are the arithmetic, not a slip: at M = 1 an output is ONE product, which fp32 rounds once (2^-24 = 6.0e-8) while three
    bf16 pieces per operand and six of their nine products leave up to 2^-23 of it out and round five partial sums
    (csrc/gemm_bx3.hip: "relative error of a product 2^-22" = 2.4e-7).  From M = 70 on the bf16 x 3 figures are at most 2.32e-7
    ((161, 192, 65); e32 2.33e-7) and within 1.04 x e32; the fp32 kernel's within 1.29 x e32."""
    worst = 0.0
    for c in C.TN_CASES:
        got = _tn_call(lib, c, arith)
        worst = max(worst, _tn_hold("E %s arith %d" % (c.name, arith), got, c, 1.0, 0))
    print("GK| worst E arith %d: %.2e" % (arith, worst))


@pytest.mark.parametrize("arith", [0, 1])
def test_gemm_tn_alpha_and_accumulate(lib, arith):
    """E.  alpha 1, -0.5, 1/3 x accumulate 0, 1 (into a pre-filled out) on one shape per kernel.
    measured, worst: 1.57e-7 (e32 1.86e-7) at (161, 257, 33), alpha 1 with accumulate, fp32; 1.53e-7 in bf16 x 3 there."""
    for c in (c for c in C.TN_CASES if c.name in C.TN_EPILOGUE):
        for alpha in C.TN_ALPHAS:
            for acc in (0, 1):
                got = _tn_call(lib, c, arith, alpha, acc)
                _tn_hold("E %s alpha %.3f acc %d arith %d" % (c.name, alpha, acc, arith), got, c, alpha, acc)


# ----------------------------------------------------------------------------------------------------------------------
# the layout helpers of csrc/gemm.hip (32 x 32 LDS tile transposes)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", [1, 9, 33, 64])
def test_layout_copies_are_exact_each_way(lib, C_):
    """r3d_cm_to_pm and r3d_pm_to_cm, each against the host transpose by itself (no round trip): B = 3, N on both sides of
    the 32-point tile, one point, many tiles; the point-major side has ld > C inside poison; exact copies."""
    B = 3
    for N in (1, 31, 32, 33, 500):
        x = torch.from_numpy(_rs(97 * C_ + N).randn(B, C_, N).astype(np.float32))      # channel-major
        want_pm = x.permute(0, 2, 1).reshape(B * N, C_).contiguous()
        ld = C_ + 5
        cm = _vec(x.reshape(-1))
        pm = Slab(B * N, C_, ld, 2)
        _check(lib.r3d_cm_to_pm(_p(cm.view), B, C_, N, _p(pm.view), ld, _st()))
        torch.cuda.synchronize()
        assert pm.rest_intact() and cm.rest_intact()
        assert _same_bits(pm.host(), want_pm), (C_, N)
        src = Slab(B * N, C_, ld, 2, want_pm)
        dst = Slab(1, B * C_ * N, B * C_ * N, 0, rows=1)
        _check(lib.r3d_pm_to_cm(_p(src.view), ld, B, C_, N, _p(dst.view), _st()))
        torch.cuda.synchronize()
        assert dst.rest_intact() and src.rest_intact()
        assert _same_bits(dst.host().reshape(B, C_, N), x), (C_, N)
