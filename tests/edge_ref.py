"""Float64 restatement of the training-mode EdgeConv layer (csrc/edgeconv_train.hip, edgeconv_bwd_bx3.h), segment by
segment, for tests/test_gpu_edge_train.py; tests/test_edge_ref_host.py holds it to torch autograd in float64 on the
reference's own formulation (models/dgcnn.py:26-61 with nn.BatchNorm2d in train mode) without a GPU.

Formulas (the header comment of edgeconv_train.hip), with PQ = [P | Q] (M, 128) the raw point-wise GEMM and idx (B, N, K)
neighbour positions inside each cloud (clamped to the cloud, as every kernel does):
    e1(i,t) = P[j_it] + Q[i];  h1 = lrelu(s1 e1 + t1);  z2 = h1 W2^T;  out[i] = max_t lrelu(s2 z2 + t2)
    dz2 = s2 (dy2 - m1 - zhat2 m2);  dW2 = dz2^T h1;  dy1 = (dz2 W2) lrelu'(u1);  de1 = s1 (dy1 - n1 - ehat1 n2)
    dQ[i] = sum_t de1(i,t);  dP[j] = sum over the incoming edges of j of de1
BatchNorm vectors travel as bn_ref's (n_seg, 4, 64) table scale | shift | mean | invstd; statistics are per segment of an
``ops.SegLayout`` (bn_ref.seg_slices), counts are EDGES (rows x K).

Every function takes a ``dtype``: float64 is the reference.  float32 evaluates the same formulas in fp32 on the CPU, with the
statistics summed in the KERNELS' PARTITION: partials per chunk of EC_CHUNK = 32 points of one cloud; four waves over the
points w, w + 4, ...; wave totals combined as ((0 + 1) + 2) + 3; chunks added in float64 (the z2 sums: four lane groups
over the rows 4 g .. 4 g + 3 of every 16, combined as (0 + 1) + (2 + 3)).  That is the ``e32`` the GPU tests print beside
each device error: reference arithmetic, not the code under test."""
import numpy as np
import torch

from bn_ref import F64, act_slope, bnvec_of, fold, rel, seg_counts, seg_slices  # noqa: F401  (re-exported for the tests)

EC_CHUNK = 32
F32 = torch.float32


def n_chunks(seg):
    """Statistics chunks of the layout: what r3d_edgeconv_train_ws_words counts."""
    return seg.B * (-(-seg.N // EC_CHUNK))


def cloud_segments(seg):
    """(B,) int64: the segment of every cloud."""
    out = torch.empty(seg.B, dtype=torch.int64)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        out[r0 // seg.N:r1 // seg.N] = s
    return out


def _per_cloud(table, seg, i, dtype):
    """Column i of a (n_seg, 4, 64) table as (B, 1, 1, 64), every cloud with its segment's vector."""
    return table[cloud_segments(seg), i].to(dtype)[:, None, None, :]


def _lrelu(u):
    return torch.where(u > 0, u, 0.2 * u)


def gather_e1(PQ, idx, seg, dtype=F64):
    """-> e1 (B, N, K, 64)."""
    B, N, K = idx.shape
    assert (B, N) == (seg.B, seg.N) and PQ.shape == (seg.M, 128)
    PQ = PQ.to(dtype)
    P, Q = PQ[:, :64].view(B, N, 64), PQ[:, 64:].view(B, N, 64)
    j = idx.long().clamp(0, N - 1)
    return torch.stack([P[b][j[b]] for b in range(B)]) + Q[:, :, None, :]


# ----------------------------------------------------------------------------------------------------------------------
# per-segment sums over edges, float64 or fp32 in the kernels' partition
# ----------------------------------------------------------------------------------------------------------------------
def _chunked(t, N):
    """(B, N, R, 64) numpy fp32 -> (B, cpc, 32, R, 64), the tail chunk padded with zeros (adding 0 changes no fp32 sum)."""
    B, _, R, C = t.shape
    cpc = -(-N // EC_CHUNK)
    if cpc * EC_CHUNK != N:
        t = np.concatenate((t, np.zeros((B, cpc * EC_CHUNK - N, R, C), np.float32)), 1)
    return t.reshape(B, cpc, EC_CHUNK, R, C)


def _seq(t, axis):
    """Sequential fp32 sum along an axis (np.add.accumulate adds in order)."""
    return np.take(np.add.accumulate(t, axis=axis, dtype=np.float32), -1, axis=axis)


def _seg_total(part, seg):
    """part (B, cpc, 64) fp32 chunk partials -> (n_seg, 64) fp32: a segment's chunks added in float64."""
    out = np.zeros((seg.n_seg, part.shape[-1]), np.float32)
    for s, (r0, r1) in enumerate(seg_slices(seg)):
        out[s] = part[r0 // seg.N:r1 // seg.N].astype(np.float64).sum((0, 1)).astype(np.float32)
    return out


def edge_sums_f32(t, seg, mode="waves"):
    """Per-segment sum over edges of t (B, N, K, 64) fp32, as the kernels form it.
    "waves":  wave w adds the edges of points w, w + 4, ... of the chunk one after the other (r3d_edge_stats1, the
              sum dy1 ehat1 of r3d_edgeconv_bwd1_kernel);
    "points": the same waves over per-point sums formed first (sum dy1 of r3d_edgeconv_bwd1_kernel);
    "rows":   lane group g adds rows 16 t + 4 g + i of every 4-point unit in order, groups meet as (0 + 1) + (2 + 3)
              (the z2 sums of r3d_edgeconv_train_fwd2_kernel)."""
    t = t.numpy() if isinstance(t, torch.Tensor) else t
    B, N, K, C = t.shape
    c = _chunked(t.astype(np.float32, copy=False), N)  # (B, cpc, 32, K, C)
    cpc = c.shape[1]
    if mode == "rows":
        u = c.reshape(B, cpc, 8, K // 4, 4, 4, C)                      # unit, t, g, i  (row 16 t + 4 g + i of 4 K rows)
        u = u.transpose(0, 1, 4, 2, 3, 5, 6).reshape(B, cpc, 4, -1, C)  # g | unit, t, i
        g = _seq(u, 3)
        part = (g[:, :, 0] + g[:, :, 1]) + (g[:, :, 2] + g[:, :, 3])
    else:
        w = c.reshape(B, cpc, 8, 4, K, C).transpose(0, 1, 3, 2, 4, 5)   # wave | its points | t
        if mode == "points":
            w = _seq(w, 4)                                              # per-point sums first
            w = _seq(w, 3)
        else:
            w = _seq(w.reshape(B, cpc, 4, 8 * K, C), 3)
        part = ((w[:, :, 0] + w[:, :, 1]) + w[:, :, 2]) + w[:, :, 3]
    return torch.from_numpy(_seg_total(part, seg))


def edge_sums(t, seg, dtype=F64, mode="waves"):
    """-> (sums (n_seg, 64), terms (n_seg, 64) = sums of |t|) over the edges of every segment."""
    terms = torch.stack([t[r0 // seg.N:r1 // seg.N].abs().sum((0, 1, 2), dtype=F64) for r0, r1 in seg_slices(seg)])
    if dtype == F32:
        return edge_sums_f32(t, seg, mode), terms
    return torch.stack([t[r0 // seg.N:r1 // seg.N].sum((0, 1, 2)) for r0, r1 in seg_slices(seg)]), terms


def stats1(PQ, idx, seg, dtype=F64):
    """r3d_edge_stats1 -> dict: sums (n_seg, 2, 64) = (sum e1, sum e1^2), terms (the same of |e1|, e1^2), esum (M, 64)
    = sum_t e1 per point, esum_terms (M, 64) = sum_t |e1|."""
    e1 = gather_e1(PQ, idx, seg, dtype)
    s0, t0 = edge_sums(e1, seg, dtype)
    s1, t1 = edge_sums(e1 * e1, seg, dtype)
    if dtype == F32:
        esum = torch.from_numpy(_seq(e1.numpy(), 2))  # ps += e, t ascending
    else:
        esum = e1.sum(2)
    return dict(sums=torch.stack((s0, s1), 1), terms=torch.stack((t0, t1), 1), esum=esum.reshape(seg.M, 64),
                esum_terms=e1.abs().sum(2, dtype=F64).reshape(seg.M, 64))


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def select(zmax, zmin, argmax, argmin, bn2, seg, dtype=F64):
    """r3d_edge_select: z = zmax where scale2 >= 0, zmin otherwise, with its edge position; out = lrelu(s2 z + t2).
    -> dict: zwin, win (int64), out, out_mag = |s2 z| + |t2| (all (M, 64))."""
    rs = cloud_segments(seg).repeat_interleave(seg.N)
    s2, t2 = bn2[rs, 0].to(dtype), bn2[rs, 1].to(dtype)
    up = s2 >= 0
    z = torch.where(up, zmax.to(dtype), zmin.to(dtype))
    a = s2 * z
    return dict(zwin=z, win=torch.where(up, argmax, argmin), out=_lrelu(a + t2), out_mag=a.abs() + t2.abs())


def fwd(PQ, idx, bn1, W2, seg, bn2=None, gamma2=None, beta2=None, eps=1e-5, dtype=F64, keep_edges=True):
    """r3d_edgeconv_train_fwd_minmax (+ fold + r3d_edge_select when bn2, or gamma2 / beta2 to fold it from the z2 sums, is
    given).  -> dict: h1, z2 (B, N, K, 64; dropped with keep_edges=False), sums2 / terms2 (n_seg, 2, 64; the terms are
    those of the double sum over edges and k), zmax, zmin, argmax, argmin (M, 64; the LOWEST edge position on exact ties),
    zmag (M, 64) = max_t sum_k |h1| |W2|, gap_max / gap_min (M, 64): distance of the best z2 from the best edge of
    ANOTHER neighbour over the larger of the two magnitudes (1 where there is none); with a BatchNorm-2 table also bn2,
    zwin, win, out, out_mag."""
    B, N, K = idx.shape
    e1 = gather_e1(PQ, idx, seg, dtype)
    h1 = _lrelu(_per_cloud(bn1, seg, 0, dtype) * e1 + _per_cloud(bn1, seg, 1, dtype))
    del e1
    z2 = h1 @ W2.to(dtype).t()
    zt = h1.abs() @ W2.to(dtype).abs().t()  # the terms of z2 = sum_k h1 W2: what an error of the double sum is measured against
    s0, s1 = edge_sums(z2, seg, dtype, "rows")[0], edge_sums(z2 * z2, seg, dtype, "rows")[0]
    r = dict(sums2=torch.stack((s0, s1), 1), terms2=torch.stack((edge_sums(zt, seg)[1], edge_sums(zt * zt, seg)[1]), 1),
             zmag=zt.max(2).values.reshape(seg.M, 64).to(F64))
    del zt

    jn = idx.long().clamp(0, N - 1)
    pos_k = torch.arange(K).view(1, 1, K, 1)

    def best(z, largest):
        # first position of the extremum: the kernel scans t ascending with strict comparisons.  The gap is taken to the
        # best edge that names ANOTHER neighbour: edges of the same neighbour carry bit-equal z2 (exact ties).
        v = z.max(2).values if largest else z.min(2).values
        pos = torch.where(z == v[:, :, None, :], pos_k, K).min(2).values
        same = jn[:, :, :, None] == torch.gather(jn[:, :, :, None].expand(B, N, K, 64), 2, pos[:, :, None, :])
        fill = float("-inf") if largest else float("inf")
        zo = torch.where(same, torch.full_like(z, fill), z)
        o = zo.max(2).values if largest else zo.min(2).values
        gap = torch.where(torch.isinf(o), torch.ones_like(v), (v - o).abs() / torch.maximum(v.abs(), o.abs()).clamp_min(1e-300))
        return v.reshape(seg.M, 64), pos.reshape(seg.M, 64), gap.reshape(seg.M, 64)
    r["zmax"], r["argmax"], r["gap_max"] = best(z2, True)
    r["zmin"], r["argmin"], r["gap_min"] = best(z2, False)
    if bn2 is None and gamma2 is not None:
        bn2 = bnvec_of(fold(r["sums2"], seg_counts(seg, K), gamma2, beta2, eps)).to(dtype)
    if bn2 is not None:
        r["bn2"] = bn2
        r.update(select(r["zmax"], r["zmin"], r["argmax"], r["argmin"], bn2, seg, dtype))
    if keep_edges:
        r["h1"], r["z2"] = h1, z2
    return r


def u1_margin(PQ, idx, bn1, seg):
    """|s1 e1 + t1| / (|s1 e1| + |t1|) per edge and channel (B, N, K, 64), float64; 1 where both terms vanish."""
    a = _per_cloud(bn1, seg, 0, F64) * gather_e1(PQ, idx, seg, F64)
    b = _per_cloud(bn1, seg, 1, F64).expand_as(a)
    den = a.abs() + b.abs()
    return torch.where(den > 0, (a + b).abs() / den.clamp_min(1e-300), torch.ones_like(den))


def u2_margin(zwin, bn2, seg):
    """The same for the max-pool winner (M, 64): |s2 z + t2| / (|s2 z| + |t2|)."""
    rs = cloud_segments(seg).repeat_interleave(seg.N)
    a, b = bn2[rs, 0].to(F64) * zwin.to(F64), bn2[rs, 1].to(F64)
    den = a.abs() + b.abs()
    return torch.where(den > 0, (a + b).abs() / den.clamp_min(1e-300), torch.ones_like(den))


# ----------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------
def bwd(PQ, idx, bn1, bn2, W2, dout, argmax, seg, zwin=None, bn2_sums=None, dtype=F64, keep_edges=False):
    """r3d_edgeconv_bwd.  argmax (M, 64): the winner's edge position; its side of the LeakyReLU kink comes from zwin when
    given (what the bf16 x 3 form reads), else from the recomputed z2 (the fp32 core).  bn2_sums (n_seg, 2, 64) =
    (sum dy2, sum dy2 zhat2) as given, else summed here.  -> dict: bn2_sums, dz2, dy1 (with keep_edges), dW2 (64, 64),
    bn1_sums (n_seg, 2, 64), dP, dQ (M, 64), and *_mag for each: the sums of the absolute values of the terms."""
    B, N, K = idx.shape
    M = seg.M
    col = lambda t, i: _per_cloud(t, seg, i, dtype)
    W2 = W2.to(dtype)
    e1 = gather_e1(PQ, idx, seg, dtype)
    u1 = col(bn1, 0) * e1 + col(bn1, 1)
    eh = (e1 - col(bn1, 2)) * col(bn1, 3)
    del e1
    h1 = _lrelu(u1)
    sl1 = act_slope(u1, 2)
    del u1
    z2 = h1 @ W2.t()
    am = argmax.long().view(B, N, 1, 64)
    zw = z2.gather(2, am) if zwin is None else zwin.to(dtype).view(B, N, 1, 64)
    dwin = dout.to(dtype).view(B, N, 1, 64) * act_slope(col(bn2, 0) * zw + col(bn2, 1), 2)
    dy2 = torch.zeros_like(z2).scatter_(2, am, dwin)
    zh2 = (z2 - col(bn2, 2)) * col(bn2, 3)
    del z2
    counts = torch.tensor(seg_counts(seg, K), dtype=dtype)
    if bn2_sums is None:
        bn2_sums = torch.stack((edge_sums(dy2, seg)[0], edge_sums(dy2 * zh2, seg)[0]), 1)
    m = (bn2_sums.to(F64) / counts.to(F64)[:, None, None]).to(dtype)[cloud_segments(seg)]  # (B, 2, 64)
    m1, m2 = m[:, 0][:, None, None, :], m[:, 1][:, None, None, :]
    s2 = col(bn2, 0)
    dz2 = s2 * (dy2 - m1 - zh2 * m2)
    dz2_mag = s2.abs() * (dy2.abs() + m1.abs() + (zh2 * m2).abs())
    del dy2, zh2
    E = B * N * K
    r = dict(bn2_sums=bn2_sums)
    r["dW2"] = dz2.reshape(E, 64).t() @ h1.reshape(E, 64)
    r["dW2_mag"] = (dz2_mag.reshape(E, 64).t() @ h1.abs().reshape(E, 64)).to(F64)
    dy1 = (dz2 @ W2) * sl1
    dy1_mag = (dz2_mag @ W2.abs()) * sl1
    del h1, sl1
    a0, t0 = edge_sums(dy1, seg, dtype, "points")
    a1, t1 = edge_sums(dy1 * eh, seg, dtype, "waves")
    r["bn1_sums"] = torch.stack((a0, a1), 1)
    r["bn1_sums_mag"] = torch.stack((edge_sums(dy1_mag, seg)[0], edge_sums(dy1_mag * eh.abs(), seg)[0]), 1).to(F64)
    n = (r["bn1_sums"].to(F64) / counts.to(F64)[:, None, None]).to(dtype)[cloud_segments(seg)]
    n1, n2 = n[:, 0][:, None, None, :], n[:, 1][:, None, None, :]
    s1 = col(bn1, 0)
    de1 = s1 * (dy1 - n1 - eh * n2)
    de1_mag = s1.abs() * (dy1_mag + n1.abs() + (eh * n2).abs())
    r["dQ"], r["dQ_mag"] = de1.sum(2).reshape(M, 64), de1_mag.sum(2).reshape(M, 64).to(F64)
    tgt = (idx.long().clamp(0, N - 1) + N * torch.arange(B)[:, None, None]).reshape(-1)
    r["dP"] = torch.zeros(M, 64, dtype=dtype).index_add_(0, tgt, de1.reshape(E, 64))
    r["dP_mag"] = torch.zeros(M, 64, dtype=dtype).index_add_(0, tgt, de1_mag.reshape(E, 64)).to(F64)
    if keep_edges:
        r["dz2"], r["dz2_mag"], r["dy1"], r["dy1_mag"] = dz2, dz2_mag, dy1, dy1_mag
    return r


def kink_edges(PQ, idx, bn1, seg, margin):
    """-> (exempt_Q, exempt_P) (M, 64) bool: the dQ / dP elements one of whose edges has u1_margin < margin."""
    B, N, K = idx.shape
    near = u1_margin(PQ, idx, bn1, seg) < margin
    tgt = (idx.long().clamp(0, N - 1) + N * torch.arange(B)[:, None, None]).reshape(-1)
    hitP = torch.zeros(seg.M, 64).index_add_(0, tgt, near.reshape(-1, 64).float()) > 0
    return near.any(2).reshape(seg.M, 64), hitP
