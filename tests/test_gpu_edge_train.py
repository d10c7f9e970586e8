"""The training-mode EdgeConv kernels, one at a time and as a layer, against float64: r3d_edge_stats1,
r3d_edgeconv_train_fwd_minmax, r3d_edge_select, r3d_edgeconv_bwd in both matrix arithmetics (csrc/edgeconv_train.hip,
edgeconv_bwd_bx3.h) through the C ABI, and train_ops.edgeconv_train_fwd / edgeconv_train_bwd over them.

Reference: tests/edge_ref.py (float64, segment by segment; held to torch autograd in tests/test_edge_ref_host.py).  Cases:
tests/edge_cases.py.  Inputs are INJECTED, not chained: every kernel gets the reference's own upstream results rounded to
fp32 (BatchNorm tables folded in float64, argmax, zwin, esum, bn2_sums), so no winner flip and no upstream error enters a
dependent kernel's figure.  rev_ws comes from r3d_edge_reverse after it is found equal to the stable sort.

What is compared how.  Sums: |got - ref| / sum |terms| per segment and channel.  Values: |got - ref| / mag per element,
mag the sum of the absolute values of the element's terms.  Winners: equal to the reference wherever the best z2 lies more
than 64 ULP (relative) from the best z2 of ANOTHER neighbour -- edges that name the same neighbour carry bit-equal z2 and
must give the lowest position ("repeats" lists).  LeakyReLU kinks: a dQ / dP element one of whose edges has
|u1| < 1e-5 (|s1 e1| + |t1|) is exempt; a winner that close to LeakyReLU-2's kink gets dout = 0 on the host.  The shares
are capped (0.5 % / 1 %) and asserted on the reference in tests/test_edge_ref_host.py.  dW2 and bn1_sums are compared
in full.  Every output buffer is exactly as large as include/r3d.h says, with guard words behind it; dPQ starts as NaN.

Bars.  Each test prints ``EC| case quantity err e32 bar``: err the device against float64, e32 the same formulas in fp32
on the CPU with the statistics in the kernels' partition against float64.  bar = 4 x the worst e32 over this module's
cases (the margin covers the MFMA's accumulation order against the restatement's), never above its ceiling: 8e-6 of the
summed terms for statistics, 1e-4 for out / zmax / zmin, 5e-4 for dW2 and dPQ.  The bf16 x 3 form is held to the same
bars as the fp32 core."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import edge_cases as EC
import edge_ref as R

pytestmark = pytest.mark.gpu

SENT = -77.25
F32 = torch.float32
CEIL_SUM, CEIL_FEAT, CEIL_GRAD = 8e-6, 1e-4, 5e-4
# quantity -> bar = min(4 x worst e32 over this module's cases, ceiling); beside each: worst figure on the MI355X (fp32
# core | bf16 x 3 where they differ) | worst e32, and the case that set the e32.  The statistics, esum and out come out
# bit for bit as the restatement's.  The family channels at mean 0 / 8 sigma / 30 sigma, worst over the cases:
#   dQ  fp32 core 2.72e-7 / 3.59e-7 / 2.95e-7   bf16 x 3 3.41e-7 / 2.33e-7 / 3.01e-7   (e32 2.88e-7 / 2.71e-7 / 3.12e-7)
#   dP  fp32 core 4.49e-7 / 4.27e-7 / 5.84e-7   bf16 x 3 3.66e-7 / 4.22e-7 / 5.84e-7   (e32 4.02e-7 / 5.57e-7 / 4.40e-7)
#   var_K of r3d_edge_stats1's sums  1.21 / 4.44 / 2.91 (the e32 figures are the same)
# Both arithmetics hold the common bar at 30 sigma: bwd2's (esum - K mu1) invstd1 needs no other form.
BAR = dict(
    sum1=1.54e-6,         # 3.84e-7 | 3.84e-7   1-1-0-8-K32-hubs       ceiling 8e-6
    esum=1.27e-6,         # 3.16e-7 | 3.16e-7   2-3-1-36-K20-perm      ceiling 8e-6
    var_K=17.8,           # 4.44 | 4.44      2-3-1-36-K20-hubs      ceiling 194
    sum2=6.97e-6,         # 1.74e-6 | 1.74e-6   1-1-0-8-K4-perm        ceiling 8e-6 (of the terms of sum_e sum_k h1 W2)
    zext=7.77e-6,         # 2.00e-6 | 1.94e-6   1-1-0-8-K4-repeats     ceiling 1e-4
    out=4.64e-7,          # 1.16e-7 | 1.16e-7   11-8-3-1064-K4-perm    ceiling 1e-4
    dW2=1.55e-5,          # 3.89e-6 | 3.82e-6 | 3.85e-6   1-1-0-8-K4-perm        ceiling 5e-4
    bn1_sums=1.48e-6,     # 3.79e-7 | 3.79e-7 | 3.68e-7   1-1-0-8-K4-perm        ceiling 8e-6
    dP=2.50e-6,           # 6.68e-7 | 5.84e-7 | 6.23e-7   11-8-3-1064-K4-perm    ceiling 5e-4
    dQ=1.91e-6,           # 4.46e-7 | 3.53e-7 | 4.75e-7   11-8-3-1064-K4-perm    ceiling 5e-4
    L_out=1.30e-6,        # 3.44e-7 | 4.23e-7 | 3.24e-7   (2,3,1,36) K20 C9      ceiling 1e-4
    L_dW1=1.88e-6,        # 3.98e-7 | 3.98e-7 | 4.69e-7   (2,3,1,36) K20 C9      ceiling 5e-4
    L_dW2=2.80e-6,        # 7.42e-7 | 7.20e-7 | 6.99e-7   (2,1,3,40) K20 C64
    L_dg=1.79e-6,         # 4.94e-7 | 4.94e-7 | 4.46e-7   (2,1,3,40) K20 C64
    L_db=2.41e-6,         # 5.14e-7 | 1.16e-6 | 6.00e-7   (2,3,1,36) K20 C9
    L_dx=2.16e-6,         # 3.63e-7 | 3.65e-7 | 5.38e-7   (2,3,1,36) K20 C9
)
assert max(BAR[k] for k in ("sum1", "esum", "sum2", "bn1_sums")) <= CEIL_SUM
assert max(BAR[k] for k in ("zext", "out", "L_out")) <= CEIL_FEAT
assert max(BAR[k] for k in ("dW2", "dP", "dQ", "L_dW1", "L_dW2", "L_dg", "L_db", "L_dx")) <= CEIL_GRAD
CEIL_VAR_K = 194.0  # as tests/test_gpu_bn_train.py: 2 (storage) + 1.5 x 128 additions per wave partial
assert BAR["var_K"] <= CEIL_VAR_K

_ids = [EC.case_id(c) for c in EC.CASES]


@pytest.fixture(scope="module")
def env():
    from r3dfsseg_amd import _lib, ops, train_ops
    return SimpleNamespace(lib=_lib.load(), _lib=_lib, ops=ops, T=train_ops, dev=torch.device("cuda"))


class Hold:
    """Prints every figure of a test, then fails on the first one above its bar."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def __call__(self, what, err, e32, bar):
        print("EC| %-24s %-22s err %.3e  e32 %.3e  bar %.3e" % (self.case, what, err, e32, bar))
        if not err <= bar:
            self.bad.append((what, err, bar))

    def note(self, what, err, e32):
        print("EC| %-24s %-22s err %.3e  e32 %.3e  (reported)" % (self.case, what, err, e32))

    def done(self):
        assert not self.bad, (self.case, self.bad)


class Guarded:
    """n elements exactly, 64 guard words behind them."""

    def __init__(self, n, dev, dtype=F32, fill=None):
        self.full = torch.full((n + 64,), SENT if dtype == F32 else -77, device=dev, dtype=dtype)
        self.t = self.full[:n]
        if fill is not None:
            self.t.fill_(fill)

    def ok(self):
        return bool((self.full[self.t.numel():] == (SENT if self.full.dtype == F32 else -77)).all())


def _ws(env, seg):
    words = env.lib.r3d_edgeconv_train_ws_words(seg.B, seg.N)
    chunks = (words - 64 - 1024 * 4096) // 128
    # the partition the layout was chosen for (an episode run alone is not in the table)
    assert chunks == R.n_chunks(seg) == EC.CHUNKS.get((seg.E, seg.S, seg.Q, seg.N), chunks)
    return Guarded(words, env.dev)


def _table(env, seg, table):
    bn = env.T.BNVec(seg.n_seg, 64, env.dev)
    bn.t.copy_(table.to(env.dev))
    return bn


def _sub(c, e=0):
    """Episode e of a case alone: (layout, row slice, cloud slice, segment slice)."""
    from r3dfsseg_amd.ops import SegLayout
    seg = c["seg"]
    one = SegLayout(1, seg.S, seg.Q, seg.N)
    per = seg.n_seg // seg.E
    return one, slice(e * seg.ep_rows, (e + 1) * seg.ep_rows), slice(e * seg.clouds, (e + 1) * seg.clouds), slice(e * per, (e + 1) * per)


def _sum_err(got, ref, terms):
    e = (got.double() - ref.double()).abs() / terms.double().clamp_min(1e-300)
    assert bool((got.double()[terms == 0] == ref.double()[terms == 0]).all())
    return float(e[terms > 0].max()) if bool((terms > 0).any()) else 0.0


def _val_err(got, ref, mag, skip=None):
    e = (got.double() - ref.double()).abs() / mag.double().clamp_min(1e-300)
    if skip is not None:
        e = e[~skip]
    return float(e.max()) if e.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# 1. r3d_edge_stats1
# ----------------------------------------------------------------------------------------------------------------------
def _dev_stats1(env, seg, K, PQ, idx):
    sums, esum, ws = Guarded(seg.n_seg * 128, env.dev), Guarded(seg.M * 64, env.dev), _ws(env, seg)
    p = env.ops._p
    env._lib.check(env.lib.r3d_edge_stats1(p(PQ), p(idx), seg.B, seg.N, K, seg.S, seg.Q, p(sums.t), p(esum.t), p(ws.t), env.ops._st()))
    torch.cuda.synchronize()
    assert sums.ok() and esum.ok() and ws.ok()
    return dict(sums=sums.t.view(seg.n_seg, 2, 64).cpu(), esum=esum.t.view(seg.M, 64).cpu())


def q_stats1(c, got):
    """quantity -> error of `got` (dict: sums, esum) against the float64 reference of case c; var_K per family channel."""
    st, seg = c["st"], c["seg"]
    q = dict(sum1=_sum_err(got["sums"], st["sums"], st["terms"]), esum=_val_err(got["esum"], st["esum"], st["esum_terms"]))
    n = torch.tensor(c["counts"], dtype=R.F64)[:, None]
    var = lambda s: s[:, 1].double() / n - (s[:, 0].double() / n) ** 2
    mean = st["sums"][:, 0] / n
    unit = (var(st["sums"]) + mean * mean) * 2.0 ** -23
    k = (var(got["sums"]) - var(st["sums"])).abs() / unit
    for ch, m in zip(EC.FAMILY, EC.FAMILY_MEAN):
        q["var_K@%g" % m] = float(k[:, ch].max())
    q["var_K"] = max(q["var_K@%g" % m] for m in EC.FAMILY_MEAN)
    return q


def f32_stats1(c):
    return R.stats1(c["PQ"], c["idx"], c["seg"], F32)


@pytest.mark.parametrize("cs", EC.CASES, ids=_ids)
def test_edge_stats1_against_float64(env, cs):
    """(sum e1, sum e1^2) per segment and the per-point esum; the variance on the family channels at mean 0 / 8 sigma /
    30 sigma in units of (sigma^2 + mean^2) 2^-23; bit-identical from run to run, and an episode inside a batch gives the
    bits it gives alone (the several-chunks case: workgroups take several chunks)."""
    c = EC.case(*cs)
    seg, K = c["seg"], c["K"]
    h = Hold(EC.case_id(cs))
    PQ, idx = c["PQ"].to(env.dev), c["idx"].to(env.dev)
    got = _dev_stats1(env, seg, K, PQ, idx)
    q, e32 = q_stats1(c, got), q_stats1(c, f32_stats1(c))
    for k in ("sum1", "esum", "var_K"):
        h(k, q[k], e32[k], BAR[k])
    for m in EC.FAMILY_MEAN:
        h.note("var_K@%g" % m, q["var_K@%g" % m], e32["var_K@%g" % m])
    again = _dev_stats1(env, seg, K, PQ, idx)
    assert all(torch.equal(got[k], again[k]) for k in got)
    if seg.E > 1:
        one, rows, clouds, segs = _sub(c)
        alone = _dev_stats1(env, one, K, PQ[rows], idx[clouds])
        assert torch.equal(alone["sums"], got["sums"][segs]) and torch.equal(alone["esum"], got["esum"][rows])
    h.done()


# ----------------------------------------------------------------------------------------------------------------------
# 2. r3d_edgeconv_train_fwd_minmax
# ----------------------------------------------------------------------------------------------------------------------
def _dev_fwd(env, seg, K, PQ, idx, bn1, W2):
    M = seg.M
    o = dict(zmax=Guarded(M * 64, env.dev), zmin=Guarded(M * 64, env.dev), argmax=Guarded(M * 64, env.dev, torch.int32),
             argmin=Guarded(M * 64, env.dev, torch.int32), sums2=Guarded(seg.n_seg * 128, env.dev))
    ws = _ws(env, seg)
    p = env.ops._p
    s1, t1, _, _ = bn1.ptrs()
    env._lib.check(env.lib.r3d_edgeconv_train_fwd_minmax(p(PQ), p(idx), s1, t1, bn1.stride, p(W2), seg.B, seg.N, K, seg.S, seg.Q,
                                                         p(o["zmax"].t), p(o["zmin"].t), p(o["argmax"].t), p(o["argmin"].t),
                                                         p(o["sums2"].t), p(ws.t), env.ops._st()))
    torch.cuda.synchronize()
    assert ws.ok() and all(g.ok() for g in o.values())
    return {k: g.t.view(seg.n_seg, 2, 64).cpu() if k == "sums2" else g.t.view(M, 64).cpu() for k, g in o.items()}


def q_fwd(c, got):
    fw = c["fw"]
    q = dict(sum2=_sum_err(got["sums2"], fw["sums2"], fw["terms2"]),
             zext=max(_val_err(got["zmax"], fw["zmax"], fw["zmag"]), _val_err(got["zmin"], fw["zmin"], fw["zmag"])))
    for k, gap in (("argmax", "gap_max"), ("argmin", "gap_min")):
        clear = fw[gap] >= EC.GAP
        q[k] = int((got[k].long()[clear] != fw[k][clear]).sum())  # winners that differ where the gap is clear
    return q


def f32_fwd(c):
    return R.fwd(c["PQ"], c["idx"], c["bn1"], c["W2"], c["seg"], dtype=F32, keep_edges=False)


@pytest.mark.parametrize("cs", EC.CASES, ids=_ids)
def test_fwd_minmax_against_float64(env, cs):
    """z2 sums per segment, zmax / zmin and their positions on the reference's BatchNorm-1 table: positions equal wherever
    the gap is clear, the LOWEST position among bit-equal z2; run to run and alone / in a batch the same bits."""
    c = EC.case(*cs)
    seg, K = c["seg"], c["K"]
    h = Hold(EC.case_id(cs))
    PQ, idx, W2 = c["PQ"].to(env.dev), c["idx"].to(env.dev), c["W2"].to(env.dev)
    bn1 = _table(env, seg, c["bn1"])
    got = _dev_fwd(env, seg, K, PQ, idx, bn1, W2)
    q, e32 = q_fwd(c, got), q_fwd(c, f32_fwd(c))
    for k in ("sum2", "zext"):
        h(k, q[k], e32[k], BAR[k])
    h("winners that differ", q["argmax"] + q["argmin"], e32["argmax"] + e32["argmin"], 0)
    assert int(got["argmax"].min()) >= 0 and int(got["argmax"].max()) < K and int(got["argmin"].min()) >= 0 and int(got["argmin"].max()) < K
    if c["kind"] == "repeats":  # every neighbour is named twice: the winner is always the first of two bit-equal z2
        j = c["idx"].long()
        for k in ("argmax", "argmin"):
            a = got[k].long().view(seg.B, seg.N, 64)
            wj = torch.gather(j[:, :, :, None].expand(-1, -1, -1, 64), 2, a[:, :, None, :])
            earlier = (j[:, :, :, None] == wj) & (torch.arange(K).view(1, 1, K, 1) < a[:, :, None, :])
            assert not bool(earlier.any()), k
    again = _dev_fwd(env, seg, K, PQ, idx, bn1, W2)
    assert all(torch.equal(got[k], again[k]) for k in got)
    if seg.E > 1:
        one, rows, clouds, segs = _sub(c)
        alone = _dev_fwd(env, one, K, PQ[rows], idx[clouds], _table(env, one, c["bn1"][segs]), W2)
        assert all(torch.equal(alone[k], got[k][segs if k == "sums2" else rows]) for k in got)
    h.done()


# ----------------------------------------------------------------------------------------------------------------------
# 3. r3d_edge_select
# ----------------------------------------------------------------------------------------------------------------------
def _embed(t, form, dev):
    """t (M, 64) as the encoder passes operands: 0 contiguous; 1 columns 64..127 of a 192-wide buffer; 2 columns 1..64 of a
    67-wide buffer (rows not 16-byte aligned).  The rest of the buffer holds SENT.  -> (view, buffer, column offset)."""
    off, ld = ((0, 64), (64, 192), (1, 67))[form]
    buf = torch.full((t.shape[0], ld), SENT, device=dev)
    buf[:, off:off + 64] = t.to(dev)
    return buf[:, off:off + 64], buf, off


def _padding_untouched(buf, off):
    return bool((buf[:, :off] == SENT).all()) and bool((buf[:, off + 64:] == SENT).all())


def f32_select(c):
    fw = c["fw"]
    return R.select(fw["zmax"].float(), fw["zmin"].float(), fw["argmax"], fw["argmin"], c["bn2"], c["seg"], F32)


@pytest.mark.parametrize("cs", EC.CASES, ids=_ids)
def test_edge_select_against_float64(env, cs):
    """On the reference's zmax / zmin / positions (fp32) and BatchNorm-2 table: the selected z and its position IN PLACE,
    exactly; out against float64, contiguous and as a 64-column slice of a 192-wide buffer whose padding stays."""
    c = EC.case(*cs)
    seg, fw, sel = c["seg"], c["fw"], c["sel"]
    M = seg.M
    h = Hold(EC.case_id(cs))
    bn2 = _table(env, seg, c["bn2"])
    s2, t2, _, _ = bn2.ptrs()
    p = env.ops._p
    outs = []
    for form in (0, 1):
        zmax, argmax = Guarded(M * 64, env.dev), Guarded(M * 64, env.dev, torch.int32)
        zmax.t.copy_(fw["zmax"].float().reshape(-1).to(env.dev))
        argmax.t.copy_(fw["argmax"].int().reshape(-1).to(env.dev))
        zmin, argmin = fw["zmin"].float().to(env.dev), fw["argmin"].int().to(env.dev)
        out, buf, off = _embed(torch.full((M, 64), SENT), form, env.dev)
        env._lib.check(env.lib.r3d_edge_select(p(zmax.t), p(zmin), p(argmax.t), p(argmin), s2, t2, bn2.stride, M, seg.rows_a,
                                               seg.rows_b, p(out), out.stride(0), env.ops._st()))
        torch.cuda.synchronize()
        assert zmax.ok() and argmax.ok() and _padding_untouched(buf, off)
        assert torch.equal(zmax.t.view(M, 64).cpu(), c["zwin32"]) and torch.equal(argmax.t.view(M, 64).cpu().long(), sel["win"])
        assert torch.equal(zmin.cpu(), fw["zmin"].float()) and torch.equal(argmin.cpu(), fw["argmin"].int())
        outs.append(out.contiguous().cpu())
    assert torch.equal(outs[0], outs[1])
    ref = R.select(fw["zmax"].float(), fw["zmin"].float(), fw["argmax"], fw["argmin"], c["bn2"], seg)  # float64 on the fp32 inputs
    h("out", _val_err(outs[0], ref["out"], ref["out_mag"]), _val_err(f32_select(c)["out"], ref["out"], ref["out_mag"]), BAR["out"])
    h.done()


# ----------------------------------------------------------------------------------------------------------------------
# 4. r3d_edgeconv_bwd
# ----------------------------------------------------------------------------------------------------------------------
def _reverse(env, idx):
    """rev_ws of r3d_edge_reverse, asserted equal to the stable sort (as tests/test_gpu_edge_reverse.py)."""
    B, N, K = idx.shape
    ws = torch.full((env.lib.r3d_edge_reverse_ws_words(B, N, K),), -7, device=env.dev, dtype=torch.int32)
    env._lib.check(env.lib.r3d_edge_reverse(env.ops._p(idx), B, N, K, env.ops._p(ws), ws.numel(), env.ops._st()))
    torch.cuda.synchronize()
    got = ws.cpu().numpy()
    tgt = (np.clip(idx.cpu().numpy(), 0, N - 1) + np.arange(B)[:, None, None] * N).reshape(-1)
    order = np.argsort(tgt, kind="stable")
    ptr = np.searchsorted(tgt[order], np.arange(B * N + 1), side="left")
    assert np.array_equal(got[:B * N + 1], ptr.astype(np.int32)) and np.array_equal(got[B * N + 1:B * N + 1 + B * N * K], order.astype(np.int32))
    return ws


def _dev_bwd(env, c, arith, form, want_path, part=None):
    """One r3d_edgeconv_bwd call on the injected inputs of case c (part: _sub(c) for one episode alone) under matrix
    arithmetic `arith`, dout in operand form `form`; asserts the path the call was chosen for."""
    seg, K = c["seg"], c["K"]
    rows, clouds, segs = slice(None), slice(None), slice(None)
    if part is not None:
        seg, rows, clouds, segs = part
    M = seg.M
    d, p = env.dev, env.ops._p
    PQ, idx, W2 = c["PQ"][rows].to(d), c["idx"][clouds].to(d).contiguous(), c["W2"].to(d)
    bn1, bn2 = _table(env, seg, c["bn1"][segs]), _table(env, seg, c["bn2"][segs])
    bn2_sums = EC.bn2_sums32(c)[segs].contiguous().to(d)
    dout, dbuf, off = _embed(c["dout"][rows], form, d)
    argmax, zwin = c["sel"]["win"][rows].int().to(d), c["zwin32"][rows].to(d)
    esum = c["st"]["esum"][rows].float().to(d)
    rev = _reverse(env, idx)
    o = dict(DY1=Guarded(M * K * 64, d), BE=Guarded(M * 128, d), dW2=Guarded(4096, d), bn1_sums=Guarded(seg.n_seg * 128, d),
             dPQ=Guarded(M * 128, d, fill=float("nan")))
    ws = _ws(env, seg)
    s1, t1, m1, i1 = bn1.ptrs()
    s2, t2, m2, i2 = bn2.ptrs()
    before = env.lib.r3d_get_matrix_arith()
    try:
        env._lib.check(env.lib.r3d_set_matrix_arith(arith))
        assert env.lib.r3d_debug_edgeconv_bwd_path(seg.N, dout.stride(0), dout.data_ptr() % 16, 1) == want_path
        env._lib.check(env.lib.r3d_edgeconv_bwd(p(PQ), p(idx), s1, t1, m1, i1, p(W2), s2, t2, m2, i2, bn1.stride, p(bn2_sums), p(dout),
                                                dout.stride(0), p(argmax), p(zwin), p(esum), seg.B, seg.N, K, seg.S, seg.Q,
                                                p(o["DY1"].t), p(o["BE"].t), p(rev), p(o["dW2"].t), p(o["bn1_sums"].t), p(o["dPQ"].t),
                                                p(ws.t), env.ops._st()))
        torch.cuda.synchronize()
    finally:
        env._lib.check(env.lib.r3d_set_matrix_arith(before))
    assert ws.ok() and all(g.ok() for g in o.values()) and _padding_untouched(dbuf, off)
    dPQ = o["dPQ"].t.view(M, 128).cpu()
    assert not bool(torch.isnan(dPQ).any())  # every entry written
    return dict(dW2=o["dW2"].t.view(64, 64).cpu(), bn1_sums=o["bn1_sums"].t.view(seg.n_seg, 2, 64).cpu(), dP=dPQ[:, :64].clone(),
                dQ=dPQ[:, 64:].clone())


def q_bwd(c, ref, got):
    q = dict(dW2=_val_err(got["dW2"], ref["dW2"], ref["dW2_mag"]), bn1_sums=_sum_err(got["bn1_sums"], ref["bn1_sums"], ref["bn1_sums_mag"]),
             dP=_val_err(got["dP"], ref["dP"], ref["dP_mag"], c["exP"]), dQ=_val_err(got["dQ"], ref["dQ"], ref["dQ_mag"], c["exQ"]))
    for ch, m in zip(EC.FAMILY, EC.FAMILY_MEAN):
        for k, ex in (("dP", "exP"), ("dQ", "exQ")):
            q["%s@%g" % (k, m)] = _val_err(got[k][:, ch], ref[k][:, ch], ref[k + "_mag"][:, ch], c[ex][:, ch])
    q["grad_ceiling"] = max(R.rel(got[k], ref[k]) for k in ("dW2", "dP", "dQ"))  # max over max, exempt elements included
    return q


@pytest.mark.parametrize("cs", EC.CASES, ids=_ids)
def test_edgeconv_bwd_against_float64_in_both_arithmetics(env, cs):
    """dW2, bn1_sums and dPQ on injected inputs, the fp32 core (r3d_set_matrix_arith(0)) and the default arithmetic held
    to the same bars; each call asserts the form it takes (r3d_debug_edgeconv_bwd_path): bf16 x 3 under the default when
    N % 8 == 0, the fp32 core at N = 36 and for a dout that is not 16-byte aligned (column 1 of a 67-wide buffer), where the
    default must give the bits of arithmetic 0.  dout contiguous and as a slice of a 192-wide buffer: the same bits.
    The family channels (e1 at mean 0 / 8 sigma / 30 sigma) are reported apart."""
    c = EC.case(*cs)
    seg = c["seg"]
    h = Hold(EC.case_id(cs))
    bx3 = 1 if seg.N % 8 == 0 else 0
    big = cs == EC.BIG
    ref = EC.backward(c)
    e32 = q_bwd(c, ref, EC.backward(c, F32))
    got = {0: _dev_bwd(env, c, 0, 0, 0), 1: _dev_bwd(env, c, 1, 0, bx3)}
    if bx3:
        assert not torch.equal(got[0]["dP"], got[1]["dP"])  # another arithmetic did run
    for arith in (0, 1):
        q = q_bwd(c, ref, got[arith])
        for k in ("dW2", "bn1_sums", "dP", "dQ"):
            h("a%d %s" % (arith, k), q[k], e32[k], BAR[k])
        h("a%d max over max" % arith, q["grad_ceiling"], e32["grad_ceiling"], CEIL_GRAD)
        for m in EC.FAMILY_MEAN:
            for k in ("dP", "dQ"):
                h("a%d %s@%g" % (arith, k, m), q["%s@%g" % (k, m)], e32["%s@%g" % (k, m)], BAR[k])
    del ref
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)
    assert same(got[1], _dev_bwd(env, c, 1, 0, bx3))              # run to run
    assert same(got[1], _dev_bwd(env, c, 1, 1, bx3))              # dout a slice of the 192-wide feature buffer
    if not big:
        assert same(got[0], _dev_bwd(env, c, 0, 1, 0))
        assert same(got[0], _dev_bwd(env, c, 1, 2, 0))            # misaligned dout: the default falls back to the fp32 core
        assert same(got[0], _dev_bwd(env, c, 0, 2, 0))
    if seg.E > 1:
        part = _sub(c)
        for arith in (0, 1):
            alone = _dev_bwd(env, c, arith, 0, bx3 if arith else 0, part=part)
            assert torch.equal(alone["bn1_sums"], got[arith]["bn1_sums"][part[3]])
            assert torch.equal(alone["dP"], got[arith]["dP"][part[1]]) and torch.equal(alone["dQ"], got[arith]["dQ"][part[1]])
    h.done()


# ----------------------------------------------------------------------------------------------------------------------
# 5. the layer
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer(lay, K, C):
    c = EC.layer_inputs(lay, K, C, seed=1000 * C + K + lay[3])
    return c, EC.layer_ref(c), EC.layer_ref(c, F32)


L_BAR = dict(out="L_out", dW1="L_dW1", dW2="L_dW2", dg1="L_dg", dg2="L_dg", db1="L_db", db2="L_db", dx="L_dx")


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("lay,K,C", EC.LAYER_CASES, ids=["%d-%d-%d-%d-K%d-C%d" % (l + (k, cc)) for l, k, cc in EC.LAYER_CASES])
def test_edgeconv_layer_with_segments_against_float64(env, lay, K, C, arith):
    """train_ops.edgeconv_train_fwd / edgeconv_train_bwd with seg= at the encoder's two input widths, out and dout slices
    of a 192-wide buffer: out, dW1, dW2, dgamma / dbeta of both BatchNorms and dx, max |got - ref| / max |ref|."""
    c, ref, r32 = _layer(lay, K, C)
    seg, T, d = c["seg"], env.T, env.dev
    h = Hold("a%d %s K%d C%d" % (arith, lay, K, C))
    conv1, conv2 = torch.nn.Conv2d(2 * C, 64, 1, bias=False), torch.nn.Conv2d(64, 64, 1, bias=False)
    bn1, bn2 = torch.nn.BatchNorm2d(64, eps=EC.EPS), torch.nn.BatchNorm2d(64, eps=EC.EPS)
    with torch.no_grad():
        conv1.weight.copy_(c["W1"].view(64, 2 * C, 1, 1)), conv2.weight.copy_(c["W2"].view(64, 64, 1, 1))
        bn1.weight.copy_(c["g1"]), bn1.bias.copy_(c["b1"]), bn2.weight.copy_(c["g2"]), bn2.bias.copy_(c["b2"])
    ec = SimpleNamespace(layer=[conv1.to(d), bn1.to(d).train(), None, conv2.to(d), bn2.to(d).train()])
    before = env.lib.r3d_get_matrix_arith()
    try:
        env._lib.check(env.lib.r3d_set_matrix_arith(arith))
        out, obuf, ooff = _embed(torch.full((seg.M, 64), SENT), 1, d)
        saved = T.edgeconv_train_fwd(c["x"].to(d), c["idx"].to(d).contiguous(), ec, seg.B, seg.N, out, seg)
        dout, dbuf, doff = _embed(c["dout"], 1, d)
        assert env.lib.r3d_debug_edgeconv_bwd_path(seg.N, dout.stride(0), dout.data_ptr() % 16, 1) == (arith if seg.N % 8 == 0 else 0)
        dx = torch.zeros(seg.M, C, device=d)
        dW1, dg1, db1, dW2, dg2, db2 = T.edgeconv_train_bwd(saved, dout, seg.B, seg.N, dx)
        torch.cuda.synchronize()
    finally:
        env._lib.check(env.lib.r3d_set_matrix_arith(before))
    assert _padding_untouched(obuf, ooff) and _padding_untouched(dbuf, doff)
    got = dict(out=out, dW1=dW1.reshape(64, 2 * C), dW2=dW2.reshape(64, 64), dg1=dg1, db1=db1, dg2=dg2, db2=db2, dx=dx)
    for k in ("out", "dW1", "dW2", "dg1", "db1", "dg2", "db2", "dx"):
        h(k, R.rel(got[k].detach().cpu(), ref[k]), R.rel(r32[k], ref[k]), BAR[L_BAR[k]])
    h.done()
