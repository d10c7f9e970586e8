"""Float64 restatement of the segmented Conv+BN training path (csrc/train_ops.hip, the statistics epilogues of
csrc/gemm.hip / gemm_bx3.hip, r3dfsseg_amd/train_ops.py), segment by segment, for tests/test_gpu_bn_train.py;
tests/test_bn_ref_host.py holds it to torch.nn.BatchNorm1d(...).double() in train mode without a GPU.

Everything is written over an ``ops.SegLayout`` (E episodes of [S support | Q query] clouds of N rows): segment 2 e + p
is call p of episode e when Q > 0, segment e when Q = 0.  BatchNorm vectors travel as one (n_seg, 4, C) table
scale | shift | mean | invstd, the layout of train_ops.BNVec.  Every function takes a ``dtype``: float64 is the
reference; the ``*_f32`` functions further down evaluate the same formulas in fp32 in the KERNELS' PARTITION of the
sums (the ``e32`` the GPU tests print beside each measured error: reference arithmetic, not the code under test)."""
import numpy as np
import torch

F64 = torch.float64
ULP = 2.0 ** -24  # half the spacing of fp32 numbers in [1, 2): the relative error of ONE fp32 rounding


# ------------------------------------------------------------------------------------------------------------------
# segments
# ------------------------------------------------------------------------------------------------------------------
def seg_slices(seg):
    """[(row0, row1)] of every segment, in segment order."""
    out = []
    for e in range(seg.E):
        r = e * seg.ep_rows
        out.append((r, r + seg.rows_a))
        if seg.Q:
            out.append((r + seg.rows_a, r + seg.ep_rows))
    assert len(out) == seg.n_seg and out[-1][1] == seg.M
    return out


def seg_counts(seg, per_row=1):
    """Elements per channel of every segment (per_row = K: the edges of an EdgeConv layer)."""
    return [float((r1 - r0) * per_row) for r0, r1 in seg_slices(seg)]


def row_segments(seg):
    """(M,) int64: the segment of every row."""
    out = torch.empty(seg.M, dtype=torch.int64)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        out[r0:r1] = s
    return out


# ------------------------------------------------------------------------------------------------------------------
# the formulas
# ------------------------------------------------------------------------------------------------------------------
def act_fwd(u, act):
    """act 0: identity, 1: ReLU, 2: LeakyReLU(0.2)."""
    if act == 1:
        return torch.where(u > 0, u, torch.zeros_like(u))
    if act == 2:
        return torch.where(u > 0, u, 0.2 * u)
    return u


def act_slope(u, act):
    if act == 1:
        return (u > 0).to(u.dtype)
    if act == 2:
        return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, 0.2))
    return torch.ones_like(u)


def kink_margin(Z, seg, bnvec):
    """min over all elements of |scale z + shift| / (|scale z| + |shift|): how far, relative to its terms, the nearest
    pre-activation is from the kink of ReLU / LeakyReLU (1 where both terms vanish)."""
    Z, bnvec = Z.to(F64), bnvec.to(F64)
    worst = 1.0
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        a, b = bnvec[s, 0] * Z[r0:r1], bnvec[s, 1].expand(r1 - r0, -1)
        den = a.abs() + b.abs()
        m = torch.where(den > 0, (a + b).abs() / den.clamp_min(1e-300), torch.ones_like(den))
        worst = min(worst, float(m.min()))
    return worst


def clear_kink(Z, seg, bnvec, margin):
    """Z (fp32) with every element whose pre-activation lies within `margin` (as kink_margin measures it) of the kink
    moved away from it: z -> z (1 + 8 margin), which leaves scale z + shift at ~4 margin of its terms.  The caller
    asserts kink_margin() on the result."""
    Z = Z.clone()
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        z = Z[r0:r1].to(F64)
        a, b = bnvec[s, 0].to(F64) * z, bnvec[s, 1].to(F64).expand(r1 - r0, -1)
        bad = (a + b).abs() < 2 * margin * (a.abs() + b.abs())
        Z[r0:r1] = torch.where(bad, z * (1 + 8 * margin), z).to(Z.dtype)
    return Z


def colsums(X, seg, mode=0, DY=None, bnvec=None, act=0, dtype=F64):
    """-> (sums (n_seg, 2, C), terms (n_seg, 2, C)): mode 0 (sum x, sum x^2); mode 1 (sum du, sum du zhat) with
    du = dy act'(scale z + shift), zhat = (z - mean) invstd, the segment's own vectors.  `terms`: the sums of the
    absolute values of the same terms (what a summation error is measured against)."""
    X = X.to(dtype)
    C = X.shape[1]
    sums, terms = torch.zeros(seg.n_seg, 2, C, dtype=dtype), torch.zeros(seg.n_seg, 2, C, dtype=dtype)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        x = X[r0:r1]
        if mode == 0:
            t0, t1 = x, x * x
        else:
            sc, sh, mu, is_ = (bnvec[s, i].to(dtype) for i in range(4))
            du = DY[r0:r1].to(dtype) * act_slope(sc * x + sh, act)
            t0, t1 = du, du * ((x - mu) * is_)
        sums[s, 0], sums[s, 1] = t0.sum(0), t1.sum(0)
        terms[s, 0], terms[s, 1] = t0.abs().sum(0), t1.abs().sum(0)
    return sums, terms


def fold(sums, counts, gamma, beta, eps):
    """Batch statistics -> BatchNorm vectors, from the sums AS GIVEN (fp32 sums cast to double: a comparison with
    r3d_bn_fold_seg on the same sums isolates that kernel).  counts: one per segment.  -> dict of (n_seg, C): mean,
    invstd, scale, shift, var (biased, clamped at 0), unbiased (no Bessel factor for count 1)."""
    sums, gamma, beta = sums.to(F64), gamma.to(F64), beta.to(F64)
    n = torch.tensor(counts, dtype=F64)[:, None]
    mean = sums[:, 0] / n
    var = (sums[:, 1] / n - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma[None] * invstd
    shift = beta[None] - mean * scale
    unb = torch.where(n > 1, var * n / (n - 1).clamp_min(1.0), var)
    return dict(mean=mean, invstd=invstd, scale=scale, shift=shift, var=var, unbiased=unb)


def bnvec_of(f):
    """The (n_seg, 4, C) table of a fold() result."""
    return torch.stack((f["scale"], f["shift"], f["mean"], f["invstd"]), 1)


def running(rm, rv, records, momentum, bias=None):
    """nn.BatchNorm's running-statistics update, record after record: records (n, 2, C) = (batch mean, unbiased batch
    variance); a conv bias in front of the BatchNorm is added to each batch mean.  -> (running_mean, running_var)."""
    rm, rv, records = rm.to(F64).clone(), rv.to(F64).clone(), records.to(F64)
    for k in range(records.shape[0]):
        m = records[k, 0] + (bias.to(F64) if bias is not None else 0.0)
        rm = (1.0 - momentum) * rm + momentum * m
        rv = (1.0 - momentum) * rv + momentum * records[k, 1]
    return rm, rv


def affine_act(Z, seg, bnvec, act, dtype=F64):
    """-> (y (M, C) = act(scale z + shift), mag = |scale z| + |shift|)."""
    Z, bnvec = Z.to(dtype), bnvec.to(dtype)
    y, mag = torch.empty_like(Z), torch.empty_like(Z)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        a = bnvec[s, 0] * Z[r0:r1]
        y[r0:r1] = act_fwd(a + bnvec[s, 1], act)
        mag[r0:r1] = a.abs() + bnvec[s, 1].abs()
    return y, mag


def bwd_apply(Z, DY, seg, bnvec, act, sums, counts, dtype=F64):
    """dz = scale (du - sum_du / n - zhat sum_du_zhat / n) with the sums AS GIVEN.  -> (dz (M, C),
    mag = |scale| (|du| + |m1| + |zhat m2|))."""
    Z, DY, bnvec, sums = Z.to(dtype), DY.to(dtype), bnvec.to(dtype), sums.to(dtype)
    dz, mag = torch.empty_like(Z), torch.empty_like(Z)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        sc, sh, mu, is_ = bnvec[s]
        z = Z[r0:r1]
        du = DY[r0:r1] * act_slope(sc * z + sh, act)
        zh = (z - mu) * is_
        m1, m2 = sums[s, 0] / counts[s], sums[s, 1] / counts[s]
        dz[r0:r1] = sc * (du - m1 - zh * m2)
        mag[r0:r1] = sc.abs() * (du.abs() + m1.abs() + (zh * m2).abs())
    return dz, mag


# ------------------------------------------------------------------------------------------------------------------
# a whole conv + BatchNorm + activation layer
# ------------------------------------------------------------------------------------------------------------------
def layer_fwd(X, W, gamma, beta, act, seg, eps, dtype=F64):
    """z = X W^T over all rows, BatchNorm with the statistics of every segment apart, activation.  A conv bias cancels
    under batch statistics and is not part of z (it shifts the recorded mean only: running()).  -> dict: z, u (the
    pre-activation), y, bnvec (n_seg, 4, C), records (n_seg, 2, C) = (batch mean, unbiased variance), fold."""
    X, W = X.to(dtype), W.to(dtype)
    z = X @ W.t()
    sums, _ = colsums(z, seg, 0, dtype=dtype)
    f = fold(sums, seg_counts(seg), gamma, beta, eps)
    bnvec = bnvec_of(f).to(dtype)
    u = torch.empty_like(z)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        u[r0:r1] = bnvec[s, 0] * z[r0:r1] + bnvec[s, 1]
    return dict(X=X, W=W, z=z, u=u, y=act_fwd(u, act), bnvec=bnvec, records=torch.stack((f["mean"], f["unbiased"]), 1),
                fold=f, act=act, seg=seg)


def layer_bwd(fw, dY):
    """-> dict: dW, dgamma, dbeta summed over the segments; dX per row; dz."""
    seg, z, bnvec = fw["seg"], fw["z"], fw["bnvec"]
    sums, _ = colsums(z, seg, 1, DY=dY, bnvec=bnvec, act=fw["act"], dtype=z.dtype)
    dz, _ = bwd_apply(z, dY, seg, bnvec, fw["act"], sums, seg_counts(seg), dtype=z.dtype)
    return dict(dW=dz.t() @ fw["X"], dgamma=sums[:, 1].sum(0), dbeta=sums[:, 0].sum(0), dX=dz @ fw["W"], dz=dz, sums=sums)


# ------------------------------------------------------------------------------------------------------------------
# the same sums in fp32, in the kernels' partition (reference arithmetic for the e32 column of the GPU tests)
# ------------------------------------------------------------------------------------------------------------------
def ts_rows(M, C):
    """Rows per partial of r3d_colstats_seg for a segment of M rows (csrc/train_ops.hip: ~1024 workgroups whatever the
    column count, at least 64 rows, a multiple of the 32 rows of one step, at most 512)."""
    chunks = max(1, min(1024 // ((C + 63) // 64), M // 64))
    rows = -(-M // chunks)
    return min(512, -(-rows // 32) * 32)


def ts_chunks(M, C):
    return -(-M // ts_rows(M, C)) if M > 0 else 0


def _wave_chunk_sum_f32(t):
    """A chunk's fp32 partial as the column-partial kernels form it: wave w adds rows w, w + 4, ... in ascending order,
    the four wave totals meet as ((0 + 1) + 2) + 3."""
    f = np.float32
    w = [np.add.accumulate(t[k::4], axis=0, dtype=f)[-1] if t[k::4].shape[0] else np.zeros(t.shape[1], f) for k in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


def colsums_f32(X, seg, mode=0, DY=None, bnvec=None, act=0, tile=None):
    """colsums() in fp32: every term rounded as the kernels round it (no fused multiply-add), partials per chunk of
    ts_rows() rows (tile = 64: per 64-row GEMM tile, the epilogue statistics) added in fp32, the chunks in float64, the
    result rounded to fp32.  -> (n_seg, 2, C) float32."""
    f = np.float32
    X = X.numpy().astype(f)
    C = X.shape[1]
    out = np.zeros((seg.n_seg, 2, C), f)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        x = X[r0:r1]
        if mode == 0:
            t0, t1 = x, x * x
        else:
            sc, sh, mu, is_ = (bnvec[s, i].numpy().astype(f) for i in range(4))
            u = sc * x + sh
            g = DY[r0:r1].numpy().astype(f)
            du = g if act == 0 else np.where(u > 0, g, f(0) if act == 1 else f(0.2) * g).astype(f)
            t0, t1 = du, du * ((x - mu) * is_)
        rows = tile or ts_rows(r1 - r0, C)
        a, b = np.zeros(C), np.zeros(C)
        for c0 in range(0, r1 - r0, rows):
            a += _wave_chunk_sum_f32(t0[c0:c0 + rows]).astype(np.float64)
            b += _wave_chunk_sum_f32(t1[c0:c0 + rows]).astype(np.float64)
        out[s, 0], out[s, 1] = a.astype(f), b.astype(f)
    return torch.from_numpy(out)


def rel(got, want):
    """max |got - want| / max |want|."""
    return float((got.to(F64) - want.to(F64)).abs().max() / want.to(F64).abs().max().clamp_min(1e-300))
