"""The segmented Conv+BN training path, kernel by kernel and as a layer, against float64: r3d_colstats_seg,
r3d_bn_fold_seg, r3d_bn_running_update, r3d_affine_act_seg, r3d_bn_bwd_apply_seg, r3d_add_cols, r3d_copy_cols
(csrc/train_ops.hip, gemm.hip), r3d_pointwise_conv_stats_seg with its three producers of tile partials (gemm.hip,
gemm_bx3.hip), and train_ops.conv_bn_fwd / conv_bn_bwd / BNRecorder / recording() over them.

References: tests/bn_ref.py (float64, segment by segment; held to nn.BatchNorm1d.double() in tests/test_bn_ref_host.py).
Every kernel case injects its own inputs; a dependent kernel (fold, apply) is given the DEVICE's sums and is compared
with the float64 formula on those sums, so no error is carried from one stage into the next one's figure.

Layouts (E, S, Q, N) are the smallest that reach a branch each; every test asserts from r3d_colstats_seg_ws_words that
the chunk counts the layout was chosen for are the ones the library uses.  Pre-activations are kept >= MARGIN (relative
to |scale z| + |shift|) away from the activation's kink on the host, asserted, so no element is left out anywhere.

Bars.  Each test prints ``BN| case quantity err e32 bar``: err the device against float64, e32 the same formula in fp32
on the CPU in the kernel's partition against float64 (bn_ref.colsums_f32 and the fp32 dtype of the formulas).  A bar is
4 x the larger of the two worst figures over this module's cases, and never above the ceiling derived for it:
  sums      |got - ref| / sum |terms| per segment and column; ceiling 128 fp32 additions per wave partial = 8e-6
  fold      mean, invstd, scale, shift in units of ULP = 2^-24 of their magnitudes: the count of roundings (1, 1, 2, 5)
  variance  |var - var64(data)| <= K (sigma^2 + mean^2) 2^-23, i.e. relative (1 + mean^2 / sigma^2) 2^-23 K
  running   units of ULP x the largest magnitude met, per step, steps <= 10 (momentum 0.1 forgets older ones)
  affine    ULP (|scale z| + |shift|) x 3;   apply   ULP |scale| (|du| + |m1| + |zhat m2|) x 6
  layer     max |got - ref| / max |ref|; ceiling 1e-4 (the project's feature contract)
The measured figures stand beside each bar below."""
import functools
import os

import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
EPS_F32 = float(torch.tensor(EPS, dtype=torch.float32))  # the eps r3d_bn_fold_seg is handed (a float argument)
MARGIN = 1e-3        # kernel cases: distance of every pre-activation from the kink (relative to its terms)
LAYER_MARGIN = 1e-4  # layer cases
SENT = -77.25        # sentinel of padding columns, guard words and unused records
ULP = R.ULP
CEIL_SUM = 8e-6
CEIL_LAYER = 1e-4
# quantity -> bar = min(4 x the larger of the two worst figures measured over this module's cases, ceiling);
# beside each: worst figure on the MI355X | worst of the fp32 restatement on the CPU, and the case of the former
BAR = dict(
    sum0=8.9e-7,          # 2.22e-7 | 2.22e-7   (1,1,0,65) C64         ceiling 8e-6
    sum1=6.3e-7,          # 1.57e-7 | 1.57e-7   (1,1,0,31) C512        ceiling 8e-6
    conv_sum=7.5e-7,      # 1.69e-7 | 1.87e-7   bx3p (2,3,1,64) Co192; against r3d_colstats_seg 2.37e-7 (fp32, same case)
    var_K=11.4,           # 2.85 | 2.85         (5,2,0,50) C96         ceiling 194 = 2 (storage) + 1.5 x 128 additions
    mean=1.0,             # 0.99 ULP            the ceilings: one rounding each of mean and invstd, two of scale,
    invstd=1.0,           # 1.00 ULP            five of shift (4 on mean x scale, 1 on the difference)
    scale=2.0,            # 1.92 ULP
    shift=5.0,            # 3.27 ULP            (1,1,0,31) C512
    running=4.0,          # 2.07 units per step (1,1,0,65) C1024       ceiling: 3 roundings per step + the two constants
    running_bias=6.0,     # 2.07 units per step
    affine=3.0,           # 1.94 | 1.94 ULP     (3,3,1,100) C512       ceiling: product, sum, slope
    apply=6.0,            # 4.30 | 4.30 ULP     (5,2,0,50) C256        ceiling: 4.1 |du| + 4 |m1| + 6 |zhat m2|
    y=1.9e-6,             # 3.53e-7 | 4.65e-7   a0 (2,3,1,64) K64 C128 act0
    bnvec=2.4e-6,         # 5.63e-7 | 5.85e-7   a0 (3,3,1,100) K9 C64 act1
    rstat=1.3e-6,         # 3.21e-7 | 7.00e-8   a0 (3,3,1,100) K64 C128 act2
    dW=4.0e-6,            # 4.83e-7 | 9.94e-7   a0 (2,3,1,64) K64 C64 act1
    dgamma=1.5e-6,        # 2.80e-7 | 3.60e-7   a0 (2,3,1,64) K64 C64 act1
    dbeta=5.7e-7,         # 1.23e-7 | 1.42e-7   a0 (3,3,1,100) K9 C64 act1
    dX=1.9e-6,            # 4.72e-7 | 4.72e-7   a0 (3,3,1,100) K64 C128 act2
)
assert max(BAR[k] for k in ("sum0", "sum1", "conv_sum")) <= CEIL_SUM
assert max(BAR[k] for k in ("y", "bnvec", "rstat", "dW", "dgamma", "dbeta", "dX")) <= CEIL_LAYER

LAYOUTS = [(1, 1, 0, 1), (1, 1, 0, 31), (1, 1, 0, 65), (1, 1, 0, 513), (3, 3, 1, 100), (2, 1, 3, 100), (5, 2, 0, 50),
           (9, 1, 1, 40), (1, 19, 1, 64), (2, 3, 1, 64), (1, 2, 1, 64)]
# chunks of the a / b segments the layouts were chosen for (any width: the partition depends on the rows below 64 K rows)
CHUNKS = {(1, 1, 0, 1): (1, 0), (1, 1, 0, 31): (1, 0), (1, 1, 0, 65): (1, 0), (1, 1, 0, 513): (6, 0), (3, 3, 1, 100): (4, 1),
          (2, 1, 3, 100): (1, 4), (5, 2, 0, 50): (1, 0), (9, 1, 1, 40): (1, 1), (1, 19, 1, 64): (19, 1), (2, 3, 1, 64): (3, 1),
          (1, 2, 1, 64): (2, 1)}
WIDTHS = [16, 32, 64, 96, 128, 192, 256, 512, 1024]
# every layout at three widths, every width at three layouts or more; plus the pairs named for a path of their own
CASES = sorted({(lay, WIDTHS[(i + 3 * j) % 9]) for i, lay in enumerate(LAYOUTS) for j in range(3)} |
               {((3, 3, 1, 100), 1024), ((1, 1, 0, 513), 256), ((1, 19, 1, 64), 16), ((9, 1, 1, 40), 96)})
assert all(sum(1 for l, c in CASES if l == lay) >= 3 for lay in LAYOUTS)
assert all(sum(1 for l, c in CASES if c == w) >= 3 for w in WIDTHS)
_ids = lambda cases: ["%d-%d-%d-%d-C%d" % (l + (c,)) for l, c in cases]


@pytest.fixture(scope="module")
def env():
    from types import SimpleNamespace
    from r3dfsseg_amd import _lib, ops, train_ops
    return SimpleNamespace(lib=_lib.load(), _lib=_lib, ops=ops, T=train_ops, dev=torch.device("cuda"))


def _hold(case, what, err, e32, bar):
    print("BN| %-28s %-14s err %.3e  e32 %.3e  bar %.3e" % (case, what, err, e32, bar))
    assert err <= bar, (case, what, err, bar)


def _assert_chunks(env, seg, C):
    """The partition this layout was chosen for is the one the library uses (and the one bn_ref.colsums_f32 restates)."""
    one = lambda rows: (env.lib.r3d_colstats_seg_ws_words(rows, C, rows, 0) - 16) // (2 * C) if rows else 0
    ca, cb = one(seg.rows_a), one(seg.rows_b)
    assert (ca, cb) == CHUNKS[(seg.E, seg.S, seg.Q, seg.N)] == (R.ts_chunks(seg.rows_a, C), R.ts_chunks(seg.rows_b, C))
    words = env.lib.r3d_colstats_seg_ws_words(seg.M, C, seg.rows_a, seg.rows_b)
    assert words == seg.n_seg * max(ca, cb) * 2 * C + 16
    return ca, cb


@functools.lru_cache(maxsize=None)
def _case(lay, C):
    """Host inputs of a (layout, width), built once and shared: Z, DY (fp32), gamma, beta, the BatchNorm table of Z's own
    float64 statistics rounded to fp32, and the float64 results.  Columns: 0 and 1 constant (variance 0), 2 / 3 / 4 one
    family at mean 0, 8 sigma and 30 sigma, the others sigma in [0.5, 2] around a mean in [-1, 1]; gamma of both signs."""
    from r3dfsseg_amd.ops import SegLayout
    seg = SegLayout(*lay)
    g = torch.Generator().manual_seed(1000 * C + 7 * seg.M + seg.E)
    Z = torch.randn(seg.M, C, generator=g) * (0.5 + 1.5 * torch.rand(C, generator=g)) + (2 * torch.rand(C, generator=g) - 1)
    fam = torch.randn(seg.M, generator=g)
    Z[:, 0], Z[:, 1] = 1.5, 2.5
    for j, m in enumerate((0.0, 8.0, 30.0)):
        Z[:, 2 + j] = fam + m
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    beta = torch.rand(C, generator=g) - 0.5
    DY = torch.randn(seg.M, C, generator=g)
    counts = R.seg_counts(seg)
    bnvec = R.bnvec_of(R.fold(R.colsums(Z, seg, 0)[0], counts, gamma, beta, EPS)).float()
    Z = R.clear_kink(Z, seg, bnvec, MARGIN)
    assert R.kink_margin(Z, seg, bnvec) >= MARGIN  # the exclusion cap is zero: every element is compared
    return dict(seg=seg, Z=Z, DY=DY, gamma=gamma, beta=beta, bnvec=bnvec, counts=counts)


def _embed(t, form, dev):
    """t (M, C) on the device as the encoder passes operands: 0 contiguous; 1 a column slice of a wider buffer at a
    16-byte aligned offset (ld != C); 2 a slice whose offset and leading dimension are not 16-byte aligned.  The rest
    of the buffer holds SENT.  -> (view, buffer, column offset)."""
    M, C = t.shape
    off, ld = ((0, C), (64, C + 96), (1, C + 3))[form]
    buf = torch.full((M, ld), SENT, device=dev)
    buf[:, off:off + C] = t.to(dev)
    return buf[:, off:off + C], buf, off


def _padding_untouched(buf, off, C):
    return bool((buf[:, :off] == SENT).all()) and bool((buf[:, off + C:] == SENT).all())


def _bnvec_dev(env, seg, C, table):
    bn = env.T.BNVec(seg.n_seg, C, env.dev)
    bn.t.copy_(table.to(env.dev))
    return bn


def _sum_err(got, ref, terms):
    got = got.double().cpu()
    zero = terms == 0
    assert (got[zero] == 0).all()
    return float(((got - ref).abs() / terms.clamp_min(1e-300))[~zero].max()) if (~zero).any() else 0.0


# ----------------------------------------------------------------------------------------------------------------------
# 1. column sums
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay,C", CASES, ids=_ids(CASES))
def test_colstats_against_float64(env, lay, C):
    """r3d_colstats_seg, modes 0 and 1 (act 0, 1, 2), in the three operand forms.  Measured worst figures (MI355X |
    fp32 on the CPU): mode 0 2.22e-7 | 2.22e-7, mode 1 1.57e-7 | 1.57e-7: the restatement in the kernel's
    partition gives the device's figure in nearly every case."""
    c = _case(lay, C)
    seg, T = c["seg"], env.T
    _assert_chunks(env, seg, C)
    bn = _bnvec_dev(env, seg, C, c["bnvec"])
    case = "%s C%d" % (lay, C)
    Zf = [_embed(c["Z"], f, env.dev)[0] for f in range(3)]
    Gf = [_embed(c["DY"], f, env.dev)[0] for f in range(3)]
    ref, terms = R.colsums(c["Z"], seg, 0)
    got = [T.colstats(Zf[f], C, seg, mode=0) for f in range(3)]
    assert got[0].shape == (seg.n_seg, 2, C)
    _hold(case, "sum0", _sum_err(got[0], ref, terms), _sum_err(R.colsums_f32(c["Z"], seg, 0), ref, terms), BAR["sum0"])
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])  # 16 bytes per lane or 4: the same bits
    for act in (0, 1, 2):
        ref, terms = R.colsums(c["Z"], seg, 1, DY=c["DY"], bnvec=c["bnvec"], act=act)
        e32 = _sum_err(R.colsums_f32(c["Z"], seg, 1, DY=c["DY"], bnvec=c["bnvec"], act=act), ref, terms)
        got = [T.colstats(Zf[fz], C, seg, mode=1, DY=Gf[fg], bn=bn, act=act) for fz, fg in ((0, 0), (1, 1), (2, 2), (0, 2))]
        _hold(case, "sum1 act%d" % act, _sum_err(got[0], ref, terms), e32, BAR["sum1"])
        assert all(torch.equal(got[0], g_) for g_ in got[1:])


def test_colstats_stays_inside_its_workspace_and_sums(env):
    """Workspace and sums exactly as large as r3d_colstats_seg_ws_words says, guard words behind both."""
    from r3dfsseg_amd.ops import _p, _st
    for lay, C in (((3, 3, 1, 100), 128), ((1, 19, 1, 64), 1024), ((2, 1, 3, 100), 96)):
        c = _case(lay, C)
        seg = c["seg"]
        words = env.lib.r3d_colstats_seg_ws_words(seg.M, C, seg.rows_a, seg.rows_b)
        ws = torch.full((words + 64,), SENT, device=env.dev)
        sums = torch.full((seg.n_seg * 2 * C + 64,), SENT, device=env.dev)
        Z = c["Z"].to(env.dev)
        env._lib.check(env.lib.r3d_colstats_seg(_p(Z), C, None, 0, seg.M, C, seg.rows_a, seg.rows_b, 0, None, None, None, None,
                                                0, 0, _p(sums), _p(ws), _st()))
        assert (ws[words:] == SENT).all() and (sums[seg.n_seg * 2 * C:] == SENT).all()
        assert torch.equal(sums[:seg.n_seg * 2 * C].view(seg.n_seg, 2, C), env.T.colstats(Z, C, seg, mode=0))


# ----------------------------------------------------------------------------------------------------------------------
# 2. fold and running statistics
# ----------------------------------------------------------------------------------------------------------------------
def _fold_raw(env, sums, n_seg, counts, C, gamma, beta, rm=None, rv=None, rec=None, rec_index=None):
    from r3dfsseg_amd.ops import _p, _st
    bn = env.T.BNVec(n_seg, C, env.dev)
    bn.t.fill_(SENT)
    sc, sh, mu, is_ = bn.ptrs()
    env._lib.check(env.lib.r3d_bn_fold_seg(_p(sums), n_seg, counts[0], counts[1], C, _p(gamma), _p(beta), EPS, MOM, _p(rm), _p(rv),
                                           mu, is_, sc, sh, bn.stride, _p(rec), _p(rec_index), 2 * C, _st()))
    return bn


def _device_sums(env, c, C, per_row=1):
    """The device's own mode-0 sums of the case, with column 1 replaced by sums whose variance is negative before the
    clamp (mean 2.5, E x^2 = 6.25 (1 - 2^-20))."""
    seg = c["seg"]
    sums = env.T.colstats(c["Z"].to(env.dev), C, seg, mode=0)
    n = per_row * torch.tensor(c["counts"], device=env.dev, dtype=torch.float64)
    sums[:, 0, 1] = (2.5 * n).float()
    sums[:, 1, 1] = (6.25 * (1 - 2.0 ** -20) * n).float()
    return sums


@pytest.mark.parametrize("per_row", [1, 20])
@pytest.mark.parametrize("lay,C", CASES, ids=_ids(CASES))
def test_bn_fold_against_the_float64_formula(env, lay, C, per_row):
    """r3d_bn_fold_seg on the device's own sums: vectors within the count of fp32 roundings of the float64 formula on the
    SAME sums (mean 1, invstd 1, scale 2, shift 5 ULP of their terms), records (mean, unbiased variance) within 1 ULP;
    count = 20 x rows as EdgeConv folds.  The variance is then judged against the float64 variance of the DATA on
    the family columns at mean 0 / 8 sigma / 30 sigma: K (1 + mean^2 / sigma^2) 2^-23.  Measured worst figures
    (MI355X | fp32 on the CPU): K 2.85 | 2.85 at (5,2,0,50); 2.81 at (9,1,1,40); vectors 0.99, 1.00, 1.92, 3.27 ULP."""
    c = _case(lay, C)
    seg = c["seg"]
    case = "%s C%d x%d" % (lay, C, per_row)
    sums = _device_sums(env, c, C, per_row)
    counts = [n * per_row for n in c["counts"]]
    gamma, beta = c["gamma"].to(env.dev), c["beta"].to(env.dev)
    rec = torch.full((seg.n_seg, 2, C), SENT, device=env.dev)
    bn = _fold_raw(env, sums, seg.n_seg, seg.counts(per_row), C, gamma, beta, rec=rec)
    f = R.fold(sums.cpu(), counts, c["gamma"], c["beta"], EPS_F32)
    s64 = sums.double().cpu()
    n64 = torch.tensor(counts, dtype=R.F64)[:, None]
    assert (s64[:, 1, 1] / n64[:, 0] - (s64[:, 0, 1] / n64[:, 0]) ** 2 < 0).all() and (f["var"][:, 1] == 0).all()  # the clamp is met
    got = {k: getattr(bn, k).double().cpu() for k in ("mean", "invstd", "scale", "shift")}
    mag = dict(mean=f["mean"].abs(), invstd=f["invstd"], scale=f["scale"].abs(),
               shift=(c["beta"].abs()[None] + (f["mean"] * f["scale"]).abs()))
    for k in ("mean", "invstd", "scale", "shift"):
        err = float(((got[k] - f[k]).abs() / (ULP * mag[k]).clamp_min(1e-300)).max())
        _hold(case, k, err, float("nan"), BAR[k] * 1.001)
    assert float((got["invstd"][:, 1] - EPS_F32 ** -0.5).abs().max()) <= ULP * EPS_F32 ** -0.5  # variance 0: 1 / sqrt(eps)
    r = rec.double().cpu()
    assert float(((r[:, 0] - f["mean"]).abs() / (ULP * mag["mean"]).clamp_min(1e-300)).max()) <= 1.001
    assert float(((r[:, 1] - f["unbiased"]).abs() / (ULP * f["unbiased"]).clamp_min(1e-300)).max()) <= 1.001
    if per_row == 1:  # the variance against the data: the family columns
        Z = c["Z"].double()
        s32 = R.colsums_f32(c["Z"], seg, 0)
        f32 = R.fold(s32, counts, c["gamma"], c["beta"], EPS)
        K, K32 = 0.0, 0.0
        for s, (r0, r1) in enumerate(R.seg_slices(seg)):
            for col in (2, 3, 4):
                x = Z[r0:r1, col]
                m, v = float(x.mean()), float(x.var(unbiased=False))
                unb = float(r[s, 1, col])
                var_dev = unb * (r1 - r0 - 1) / (r1 - r0) if r1 - r0 > 1 else unb
                unit = (v + m * m) * 2.0 ** -23
                K, K32 = max(K, abs(var_dev - v) / unit), max(K32, abs(float(f32["var"][s, col]) - v) / unit)
        _hold(case, "var_K", K, K32, BAR["var_K"])


@pytest.mark.parametrize("lay,C", CASES[::2], ids=_ids(CASES[::2]))
def test_running_statistics_fold_records_update_and_bias(env, lay, C):
    """r3d_bn_fold_seg with running pointers == fold with records + r3d_bn_running_update without bias, bit for bit
    (include/r3d.h); both, and the update with a conv bias, within a few ULP per step of bn_ref.running; with
    rec_index_dev = 3 in a table of 2 E + 6 records only records 3 .. 3 + n_seg - 1 change.  Measured worst figures
    (units per step, see BAR): 2.07 without, 2.07 with bias."""
    from r3dfsseg_amd.ops import _p, _st
    c = _case(lay, C)
    seg, n_seg = c["seg"], c["seg"].n_seg
    case = "%s C%d" % (lay, C)
    sums = _device_sums(env, c, C)
    gamma, beta = c["gamma"].to(env.dev), c["beta"].to(env.dev)
    g = torch.Generator().manual_seed(C)
    rm0, rv0, bias = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    # (a) the fold's own running-statistics branch
    rm_a, rv_a = rm0.to(env.dev), rv0.to(env.dev)
    bn_a = _fold_raw(env, sums, n_seg, seg.counts(), C, gamma, beta, rm=rm_a, rv=rv_a)
    # (b) records at index 3 of a table of 2 E + 6, then the update
    table = torch.full((2 * seg.E + 6, 2, C), SENT, device=env.dev)
    idx = torch.tensor([3], device=env.dev, dtype=torch.int32)
    bn_b = _fold_raw(env, sums, n_seg, seg.counts(), C, gamma, beta, rec=table, rec_index=idx)
    assert torch.equal(bn_a.t, bn_b.t) and not (bn_a.t == SENT).any()
    assert (table[:3] == SENT).all() and (table[3 + n_seg:] == SENT).all() and not (table[3:3 + n_seg] == SENT).any()
    recs = table[3:3 + n_seg]
    rm_b, rv_b = rm0.to(env.dev), rv0.to(env.dev)
    env._lib.check(env.lib.r3d_bn_running_update(_p(recs), n_seg, 2 * C, C, MOM, None, _p(rm_b), _p(rv_b), _st()))
    assert torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b)
    # (c) with a conv bias
    rm_c, rv_c = rm0.to(env.dev), rv0.to(env.dev)
    bias_d = bias.to(env.dev)
    env._lib.check(env.lib.r3d_bn_running_update(_p(recs), n_seg, 2 * C, C, MOM, _p(bias_d), _p(rm_c), _p(rv_c), _st()))
    assert torch.equal(rv_c, rv_b)
    r = recs.cpu()
    steps = min(n_seg, 10)
    for what, rm, rv, b, bar in (("running", rm_b, rv_b, None, BAR["running"]), ("running_bias", rm_c, rv_c, bias, BAR["running_bias"])):
        ref_m, ref_v = R.running(rm0, rv0, r, MOM, bias=b)
        mag_m = torch.maximum(rm0.abs().double(), (r[:, 0].double() + (b.double() if b is not None else 0)).abs().max(0).values)
        if b is not None:
            mag_m = mag_m + b.abs().double()
        mag_v = torch.maximum(rv0.double(), r[:, 1].double().max(0).values)
        err = max(float(((rm.double().cpu() - ref_m).abs() / (ULP * mag_m)).max()),
                  float(((rv.double().cpu() - ref_v).abs() / (ULP * mag_v)).max())) / steps
        _hold(case, what, err, float("nan"), bar)


def _bn_module(C, gamma, beta, dev):
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM)
    bn.weight.data, bn.bias.data = gamma.clone(), beta.clone()
    bn.running_mean.data = torch.linspace(-1, 1, C)
    bn.running_var.data = torch.linspace(0.5, 2, C)
    return bn.to(dev)


@pytest.mark.parametrize("lay,K,C", [((2, 3, 1, 64), 64, 64), ((3, 3, 1, 100), 9, 128), ((9, 1, 1, 40), 64, 32)])
def test_recorder_gives_the_immediate_paths_running_statistics(env, lay, K, C):
    """recording(rec) + rec.apply(E) on conv_bn_fwd leaves the module's running statistics and num_batches_tracked bit
    for bit as the immediate update does, bias included; with update_running_stats = False nothing moves."""
    from r3dfsseg_amd.ops import SegLayout
    T = env.T
    seg = SegLayout(*lay)
    g = torch.Generator().manual_seed(K + C)
    X = torch.randn(seg.M, K, generator=g).to(env.dev)
    W = (torch.randn(C, K, generator=g) / K ** 0.5).to(env.dev)
    gamma, beta, bias = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5, torch.randn(C, generator=g).to(env.dev)
    mods = [_bn_module(C, gamma, beta, env.dev) for _ in range(3)]
    y0, _ = T.conv_bn_fwd(X, W, mods[0], 2, bias=bias, seg=seg)
    rec = T.BNRecorder(seg.E, env.dev)
    with T.recording(rec):
        y1, _ = T.conv_bn_fwd(X, W, mods[1], 2, bias=bias, seg=seg)
        assert T.bn_recorder is rec
    assert T.bn_recorder is None
    assert torch.equal(mods[1].running_mean, mods[2].running_mean) and int(mods[1].num_batches_tracked) == 0  # deferred
    rec.apply(seg.E)
    assert torch.equal(y0, y1)
    assert torch.equal(mods[0].running_mean, mods[1].running_mean) and torch.equal(mods[0].running_var, mods[1].running_var)
    assert int(mods[0].num_batches_tracked) == int(mods[1].num_batches_tracked) == seg.n_seg == 2 * seg.E
    assert not torch.equal(mods[0].running_mean, mods[2].running_mean)
    saved = T.update_running_stats
    try:
        T.update_running_stats = False
        y2, _ = T.conv_bn_fwd(X, W, mods[2], 2, bias=bias, seg=seg)
    finally:
        T.update_running_stats = saved
    assert torch.equal(y0, y2) and int(mods[2].num_batches_tracked) == 0
    assert torch.equal(mods[2].running_mean.cpu(), torch.linspace(-1, 1, C)) and torch.equal(mods[2].running_var.cpu(), torch.linspace(0.5, 2, C))


# ----------------------------------------------------------------------------------------------------------------------
# 3. element-wise passes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay,C", CASES, ids=_ids(CASES))
def test_affine_act_against_float64(env, lay, C):
    """r3d_affine_act_seg, act 0 / 1 / 2, input and output in the three operand forms: within 3 ULP of
    |scale z| + |shift| per element (its roundings: the product, the sum, 0.2f and the slope product); the padding
    columns keep their sentinel.  Measured worst figure: 1.94 ULP (the fp32 formula on the CPU: 1.94)."""
    c = _case(lay, C)
    seg = c["seg"]
    bn = _bnvec_dev(env, seg, C, c["bnvec"])
    case = "%s C%d" % (lay, C)
    for act in (0, 1, 2):
        ref, mag = R.affine_act(c["Z"], seg, c["bnvec"], act)
        e32 = float(((R.affine_act(c["Z"], seg, c["bnvec"], act, dtype=torch.float32)[0].double() - ref).abs() / (ULP * mag)).max())
        outs = []
        for fz, fo in ((0, 0), (1, 1), (2, 2), (0, 2), (1, 0)):
            Zv = _embed(c["Z"], fz, env.dev)[0]
            out, buf, off = _embed(torch.full_like(c["Z"], SENT), fo, env.dev)
            y = env.T.affine_act(Zv, bn, act, seg, out=out)
            assert y is out and _padding_untouched(buf, off, C)
            outs.append(out.contiguous())
        _hold(case, "affine act%d" % act, float(((outs[0].double().cpu() - ref).abs() / (ULP * mag)).max()), e32, BAR["affine"])
        assert all(torch.equal(outs[0], o) for o in outs[1:])
        assert torch.equal(env.T.affine_act(_embed(c["Z"], 0, env.dev)[0], bn, act, seg), outs[0])  # out=None


@pytest.mark.parametrize("per_row", [1, 20])
@pytest.mark.parametrize("lay,C", CASES, ids=_ids(CASES))
def test_bn_bwd_apply_against_float64(env, lay, C, per_row):
    """r3d_bn_bwd_apply_seg on the device's own mode-1 sums, act 0 / 1 / 2: within 6 ULP of
    |scale| (|du| + |m1| + |zhat m2|) per element; the v4 kernel (C a power of two, aligned rows) and the scalar one
    (slices that are not 16-byte aligned, aligned Z with unaligned DY among them) give the same bits at every width,
    16, 32 and 1024 included; padding columns untouched.  Measured worst figure: 4.30 ULP (the fp32 formula on the CPU: 4.30)."""
    c = _case(lay, C)
    seg = c["seg"]
    bn = _bnvec_dev(env, seg, C, c["bnvec"])
    case = "%s C%d x%d" % (lay, C, per_row)
    counts = [n * per_row for n in c["counts"]]
    for act in (0, 1, 2):
        sums = env.T.colstats(c["Z"].to(env.dev), C, seg, mode=1, DY=c["DY"].to(env.dev), bn=bn, act=act)
        ref, mag = R.bwd_apply(c["Z"], c["DY"], seg, c["bnvec"], act, sums.cpu(), counts)
        e32 = R.bwd_apply(c["Z"], c["DY"], seg, c["bnvec"], act, sums.cpu(), counts, dtype=torch.float32)[0]
        e32 = float(((e32.double() - ref).abs() / (ULP * mag).clamp_min(1e-300)).max())
        outs = []
        for fz, fg, fo in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (0, 2, 0), (1, 0, 2)):
            Zv, Gv = _embed(c["Z"], fz, env.dev)[0], _embed(c["DY"], fg, env.dev)[0]
            out, buf, off = _embed(torch.full_like(c["Z"], SENT), fo, env.dev)
            dz = env.T.bn_bwd_apply(Zv, Gv, bn, act, sums, seg.counts(per_row), seg, out=out)
            assert dz is out and _padding_untouched(buf, off, C)
            outs.append(out.contiguous())
        err = float(((outs[0].double().cpu() - ref).abs() / (ULP * mag).clamp_min(1e-300)).max())
        _hold(case, "apply act%d" % act, err, e32, BAR["apply"])
        assert all(torch.equal(outs[0], o) for o in outs[1:])  # v4 (forms 0, 1) and scalar (any operand at form 2)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 100])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 192])
def test_add_cols_and_copy_cols_are_exact(env, M, C):
    g = torch.Generator().manual_seed(M * 1000 + C)
    src_h, dst_h = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    for fs, fd in ((1, 2), (2, 1), (0, 0)):  # strided on both sides
        src = _embed(src_h, fs, env.dev)[0]
        dst, buf, off = _embed(dst_h, fd, env.dev)
        env.T.add_cols(src, dst)
        assert torch.equal(dst.cpu(), dst_h + src_h) and _padding_untouched(buf, off, C)
        dst, buf, off = _embed(dst_h, fd, env.dev)
        assert env.ops.copy_cols(src, dst) is dst
        assert torch.equal(dst.cpu(), src_h) and _padding_untouched(buf, off, C)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the GEMM's statistics epilogue, per segment, from each of the three producers of tile partials
# ----------------------------------------------------------------------------------------------------------------------
GEMM_BX3_DEFAULT = int(os.environ.get("R3D_GEMM_BX3", 7))
# producer -> (matrix arithmetic, r3d_debug_set_gemm_bx3 mask, K, row counts it takes)
PRODUCERS = {"fp32": (0, 7, 9, lambda M: True),         # r3d_pointwise_gemm_kernel (also any K % 32 != 0)
             "bx3p": (1, 7, 64, lambda M: M >= 256),    # W cut once per call: the default at M >= 256
             "bx3": (1, 3, 64, lambda M: M >= 64)}      # W cut per tile: M < 256 as it is, above with the mask without bit 2
STAT_LAYOUTS = [(1, 19, 1, 64), (2, 3, 1, 64), (1, 2, 1, 64), (1, 1, 0, 65), (1, 1, 0, 513)]
STAT_CASES = [(p, lay, Co) for p in PRODUCERS for i, lay in enumerate(STAT_LAYOUTS)
              for Co in ([32, 64, 96, 192, 512][i % 5], [32, 64, 96, 192, 512][(i + 2) % 5], [32, 64, 96, 192, 512][(i + 4) % 5])
              if PRODUCERS[p][3](lay[0] * (lay[1] + lay[2]) * lay[3])]


def _conv_stats_seg(env, X, W, seg, Co):
    from r3dfsseg_amd.ops import _p, _st
    M, K = X.shape
    words = env.lib.r3d_pointwise_conv_stats_ws_words(M, Co)
    ws = torch.full((words + 64,), SENT, device=env.dev)
    sums = torch.full((seg.n_seg * 2 * Co + 64,), SENT, device=env.dev)
    out = torch.full((M, Co), SENT, device=env.dev)
    env._lib.check(env.lib.r3d_pointwise_conv_stats_seg(_p(X), X.stride(0), _p(W), M, K, Co, _p(out), Co, seg.rows_a, seg.rows_b,
                                                        _p(sums), _p(ws), _st()))
    assert (ws[words:] == SENT).all() and (sums[seg.n_seg * 2 * Co:] == SENT).all() and not (ws[:words] == SENT).any()
    return out, sums[:seg.n_seg * 2 * Co].view(seg.n_seg, 2, Co).clone()


@pytest.mark.parametrize("producer,lay,Co", STAT_CASES, ids=["%s-%d-%d-%d-%d-Co%d" % ((p,) + l + (c,)) for p, l, c in STAT_CASES])
def test_conv_stats_seg_against_float64_sums_of_its_own_output(env, producer, lay, Co):
    """r3d_pointwise_conv_stats_seg: Out bit-equal to r3d_pointwise_conv on the same operands; the per-segment sums
    (r3d_colreduce_kernel with cmax == 0 over the producer's 64-row tile partials) against float64 sums over the
    device's own Out, and against r3d_colstats_seg(Out); an episode's sums bit-equal to the same episode alone.
    The producer is selected by (arithmetic, mask, K, M) as csrc/gemm_bx3.hip documents; that the bf16 x 3 form ran at
    all shows in Out's bits, which differ from the fp32 kernel's.  Measured worst figure (MI355X | fp32 on the CPU in
    64-row tiles): 1.69e-7 | 1.87e-7; against r3d_colstats_seg 2.37e-7."""
    from r3dfsseg_amd.ops import SegLayout
    arith, mask, K, _ = PRODUCERS[producer]
    seg = SegLayout(*lay)
    M = seg.M
    if producer == "bx3" and M < 256:
        mask = GEMM_BX3_DEFAULT  # (the default takes this kernel below 256 rows)
    g = torch.Generator().manual_seed(Co + M)
    X = (torch.randn(M, K, generator=g) + 0.5).to(env.dev)
    W = (torch.randn(Co, K, generator=g) / K ** 0.5).to(env.dev)
    before = env.lib.r3d_get_matrix_arith()
    try:
        env._lib.check(env.lib.r3d_set_matrix_arith(arith))
        env._lib.check(env.lib.r3d_debug_set_gemm_bx3(mask))
        out, sums = _conv_stats_seg(env, X, W, seg, Co)
        assert torch.equal(out, env.ops.pointwise_conv(X, W))
        alone = []
        if seg.E > 1:  # the same episodes alone
            one = SegLayout(1, seg.S, seg.Q, seg.N)
            for e in range(seg.E):
                o1, s1 = _conv_stats_seg(env, X[e * seg.ep_rows:(e + 1) * seg.ep_rows], W, one, Co)
                assert torch.equal(o1, out[e * seg.ep_rows:(e + 1) * seg.ep_rows])
                alone.append(s1)
        if arith == 1:
            env._lib.check(env.lib.r3d_set_matrix_arith(0))
            assert not torch.equal(out, env.ops.pointwise_conv(X, W))  # another arithmetic did run
    finally:
        env._lib.check(env.lib.r3d_set_matrix_arith(before))
        env._lib.check(env.lib.r3d_debug_set_gemm_bx3(GEMM_BX3_DEFAULT))
    if alone:
        assert torch.equal(torch.cat(alone), sums)
    case = "%s %s Co%d" % (producer, lay, Co)
    out_h = out.cpu()
    ref, terms = R.colsums(out_h, seg, 0)
    e32 = _sum_err(R.colsums_f32(out_h, seg, 0, tile=64), ref, terms)
    _hold(case, "conv_sum", _sum_err(sums, ref, terms), e32, BAR["conv_sum"])
    cs = env.T.colstats(out, Co, seg, mode=0)
    _hold(case, "conv_sum~colstats", _sum_err(sums, cs.double().cpu(), terms), float("nan"), BAR["conv_sum"])


def test_conv_stats_seg_refuses_segments_that_split_a_tile(env):
    from r3dfsseg_amd.ops import SegLayout, _p, _st
    seg = SegLayout(3, 3, 1, 100)
    X, W = torch.randn(seg.M, 64, device=env.dev), torch.randn(64, 64, device=env.dev)
    out, sums = torch.empty(seg.M, 64, device=env.dev), torch.empty(seg.n_seg, 2, 64, device=env.dev)
    ws = torch.empty(env.lib.r3d_pointwise_conv_stats_ws_words(seg.M, 64), device=env.dev)
    rc = env.lib.r3d_pointwise_conv_stats_seg(_p(X), 64, _p(W), seg.M, 64, 64, _p(out), 64, seg.rows_a, seg.rows_b, _p(sums), _p(ws), _st())
    assert rc != 0 and b"multiples of 64" in env.lib.r3d_last_error_string()


# ----------------------------------------------------------------------------------------------------------------------
# 5. the layer
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_case(lay, K, C, act):
    """Host inputs and float64 results of a layer case.  X is built on the host so that the float64 reference keeps every
    pre-activation LAYER_MARGIN away from the kink: rows of X that leave an element closer are moved along the weight
    row of that column (the smallest change of X that moves that z), until none is left."""
    from r3dfsseg_amd.ops import SegLayout
    seg = SegLayout(*lay)
    g = torch.Generator().manual_seed(100 * K + C + seg.M)
    X = torch.randn(seg.M, K, generator=g)
    X = torch.relu(X) * 1.3 + 0.05 * X  # (what a layer sees: the previous layer's activations)
    W = torch.randn(C, K, generator=g) / K ** 0.5
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 4 == 1, -1.0, 1.0)
    beta = 0.4 * torch.rand(C, generator=g) - 0.2
    bias = torch.randn(C, generator=g)
    dY = torch.randn(seg.M, C, generator=g)
    rowseg = R.row_segments(seg)
    for _ in range(40):
        fw = R.layer_fwd(X, W, gamma, beta, act, seg, EPS)
        if act == 0:
            break
        a, b = fw["bnvec"][rowseg, 0] * fw["z"], fw["bnvec"][rowseg, 1]
        bad = (fw["u"].abs() < 3 * LAYER_MARGIN * (a.abs() + b.abs())).nonzero()
        if bad.numel() == 0:
            break
        Xd = X.double()
        for m, c in bad.tolist():
            sc = float(fw["bnvec"][rowseg[m], 0, c])
            step = 8 * LAYER_MARGIN * float(a[m, c].abs() + b[m, c].abs()) / abs(sc) * (1.0 if float(fw["u"][m, c]) * sc >= 0 else -1.0)
            Xd[m] += step * W[c].double() / float(W[c].double().pow(2).sum())
        X = Xd.float()
    else:
        raise AssertionError("no input with the margin found")
    if act:
        margin = float((fw["u"].abs() / (a.abs() + b.abs())).min())
        assert margin >= LAYER_MARGIN, margin  # asserted on the reference before the device is looked at
    bw = R.layer_bwd(fw, dY)
    f32 = R.layer_fwd(X, W, gamma, beta, act, seg, EPS, dtype=torch.float32)
    b32 = R.layer_bwd(f32, dY)
    return dict(seg=seg, X=X, W=W, gamma=gamma, beta=beta, bias=bias, dY=dY, fw=fw, bw=bw, f32=f32, b32=b32)


LAYER_ACT = {(64, 9, 64): 2, (64, 64, 64): 1, (64, 9, 128): 1, (64, 64, 128): 0,
             (100, 9, 64): 1, (100, 64, 64): 2, (100, 9, 128): 0, (100, 64, 128): 2}  # (N, K, C) -> activation
LAYER_CASES = [(arith, lay, K, C, LAYER_ACT[(lay[3], K, C)])
               for arith in (0, 1) for lay in ((2, 3, 1, 64), (3, 3, 1, 100)) for K in (9, 64) for C in (64, 128)]


@pytest.mark.parametrize("arith,lay,K,C,act", LAYER_CASES, ids=["a%d-%d-%d-%d-%d-K%d-C%d-act%d" % ((a,) + l + (k, c, t)) for a, l, k, c, t in LAYER_CASES])
def test_conv_bn_layer_with_segments_against_float64(env, arith, lay, K, C, act):
    """conv_bn_fwd / conv_bn_bwd with seg= in both matrix arithmetics: (2,3,1,64) takes the epilogue statistics,
    (3,3,1,100) r3d_colstats_seg.  Call forms: bias=, out= a slice, dx_acc= pre-filled, want_dx=False, and the plain
    one; all must agree bit for bit where they compute the same.  Asserted against bn_ref's layer: y, the per-segment
    BatchNorm table, the running statistics (bias in the mean), dW / dgamma / dbeta summed over segments, dX per row,
    dbias exactly 0.  Measured worst figures (MI355X | fp32 on the CPU): y 3.5e-7 | 4.6e-7, table 5.6e-7 | 5.9e-7,
    running statistics 3.2e-7 | 7.0e-8, dW 4.8e-7 | 9.9e-7, dgamma 2.8e-7 | 3.6e-7, dbeta 1.2e-7 | 1.4e-7, dX 4.7e-7 | 4.7e-7."""
    T = env.T
    c = _layer_case(lay, K, C, act)
    seg, fw, bw = c["seg"], c["fw"], c["bw"]
    case = "a%d %s K%d C%d act%d" % (arith, lay, K, C, act)
    X, W, dY_h = c["X"].to(env.dev), c["W"].to(env.dev), c["dY"]
    bias = c["bias"].to(env.dev)
    before = env.lib.r3d_get_matrix_arith()
    try:
        env._lib.check(env.lib.r3d_set_matrix_arith(arith))
        # form A: bias, out a slice of a wider buffer, dY a slice, dx_acc pre-filled
        bnA = _bn_module(C, c["gamma"], c["beta"], env.dev)
        feat = torch.full((seg.M, 64 + C + 8), SENT, device=env.dev)
        yA, saved = T.conv_bn_fwd(X, W, bnA, act, bias=bias, out=feat[:, 64:64 + C], seg=seg)
        assert _padding_untouched(feat, 64, C)
        dY = _embed(dY_h, 1, env.dev)[0]
        pre = (torch.randn(seg.M, K, generator=torch.Generator().manual_seed(5)) * 0.25 * float(bw["dX"].abs().max())).float()
        acc = pre.to(env.dev)
        dW, dg, db, dbias, dX = T.conv_bn_bwd(saved, dY, want_dx=True, dx_acc=acc)
        assert dX is None and (dbias == 0).all() and dbias.shape == (C,)
        # form B: no bias, want_dx=False
        bnB = _bn_module(C, c["gamma"], c["beta"], env.dev)
        yB, savedB = T.conv_bn_fwd(X, W, bnB, act, seg=seg)
        dWB, dgB, dbB, _, dXB = T.conv_bn_bwd(savedB, dY_h.to(env.dev), want_dx=False)
        assert dXB is None and torch.equal(yB, yA) and torch.equal(dWB, dW) and torch.equal(dgB, dg) and torch.equal(dbB, db)
        assert torch.equal(savedB[3].t, saved[3].t) and torch.equal(bnA.running_var, bnB.running_var)
        # form C: dX returned
        dXC = T.conv_bn_bwd(savedB, dY_h.to(env.dev))[4]
    finally:
        env._lib.check(env.lib.r3d_set_matrix_arith(before))
    assert int(bnA.num_batches_tracked) == seg.n_seg
    h = lambda t: t.detach().double().cpu()
    rmA, rvA = R.running(torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C), fw["records"], MOM, bias=c["bias"])
    rmB, _ = R.running(torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C), fw["records"], MOM)
    rm32, rv32 = R.running(torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C), c["f32"]["records"], MOM, bias=c["bias"])
    f32, b32 = c["f32"], c["b32"]
    _hold(case, "y", R.rel(h(yA), fw["y"]), R.rel(f32["y"], fw["y"]), BAR["y"])
    for i, k in enumerate(("scale", "shift", "mean", "invstd")):
        _hold(case, "bnvec:" + k, R.rel(h(saved[3].t[:, i]), fw["bnvec"][:, i]), R.rel(f32["bnvec"][:, i], fw["bnvec"][:, i]), BAR["bnvec"])
    _hold(case, "rstat:mean+bias", R.rel(h(bnA.running_mean), rmA), R.rel(rm32, rmA), BAR["rstat"])
    _hold(case, "rstat:mean", R.rel(h(bnB.running_mean), rmB), float("nan"), BAR["rstat"])
    _hold(case, "rstat:var", R.rel(h(bnA.running_var), rvA), R.rel(rv32, rvA), BAR["rstat"])
    _hold(case, "dW", R.rel(h(dW), bw["dW"]), R.rel(b32["dW"], bw["dW"]), BAR["dW"])
    _hold(case, "dgamma", R.rel(h(dg), bw["dgamma"]), R.rel(b32["dgamma"], bw["dgamma"]), BAR["dgamma"])
    _hold(case, "dbeta", R.rel(h(db), bw["dbeta"]), R.rel(b32["dbeta"], bw["dbeta"]), BAR["dbeta"])
    _hold(case, "dX", R.rel(h(dXC), bw["dX"]), R.rel(b32["dX"], bw["dX"]), BAR["dX"])
    _hold(case, "dX:acc", R.rel(h(acc), pre.double() + bw["dX"]), R.rel(b32["dX"], bw["dX"]), BAR["dX"])
