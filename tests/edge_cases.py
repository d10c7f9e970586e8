"""The cases of tests/test_gpu_edge_train.py, built on the host from fixed seeds and shared with
tests/test_edge_ref_host.py, which asserts WITHOUT a GPU that the shares of elements the GPU tests leave out stay below
their caps -- a cap can then never hide a device failure.

A case = (layout (E, S, Q, N), K, kind of neighbour list).  Inputs are injected, not chained: PQ, idx, W2, both
BatchNorm tables folded in float64 from the float64 sums and rounded to fp32, dout, and for the backward the reference's
argmax, zwin (rounded to fp32), esum and bn2_sums.

Columns of PQ (e1 = P[j] + Q[i]): channel 0 constant e1 (variance 0); channels 2 / 3 / 4 ONE family of e1 at mean 0,
8 sigma and 30 sigma (the offset sits in the Q half); the others sigma in [0.5, 2] around a mean in [-1, 1].  gamma takes
both signs in both BatchNorms (max and min winners); |beta1| >= 0.1 keeps the constant channel off the kink.

Neighbour lists: "perm" random distinct neighbours (K > N: whole permutations one after the other), "hubs" every point
names point 0 and point N - 1 (in-degree N at two targets), "repeats" every list holds each of its neighbours twice, so two
z2 of a point are bit-equal."""
import functools

import numpy as np
import torch

import edge_ref as R

EPS = 1e-5
GAP = 64 * 2.0 ** -24   # winners are compared where the best two z2 are further apart than this, relative to their magnitude
MARGIN = 1e-5           # distance from the LeakyReLU kink (relative to the terms) below which an element is exempt
CAP_GAP = 0.005         # share of (point, channel) pairs below GAP
CAP_KINK = 0.01         # share of (point, channel) pairs exempt for MARGIN
FAMILY = (2, 3, 4)      # channels of the family; their means in sigma:
FAMILY_MEAN = (0.0, 8.0, 30.0)

BIG = ((11, 8, 3, 1064), 4, "perm")  # 4114 chunks: above every grid cap (512 / 1024 / 2048 / 4096), no multiple of 8
SMALL = [((1, 1, 0, 8), 4, "perm"), ((1, 1, 0, 8), 4, "repeats"), ((1, 1, 0, 8), 32, "hubs"),
         ((2, 3, 1, 36), 20, "perm"), ((2, 3, 1, 36), 20, "hubs"),
         ((2, 1, 3, 40), 12, "repeats"), ((2, 1, 3, 40), 20, "perm"), ((2, 1, 3, 40), 20, "hubs"),
         ((3, 2, 0, 64), 20, "perm"), ((3, 2, 0, 64), 20, "repeats")]
CASES = SMALL + [BIG]
# statistics chunks the layouts were chosen for
CHUNKS = {(1, 1, 0, 8): 1, (2, 3, 1, 36): 16, (2, 1, 3, 40): 16, (3, 2, 0, 64): 12, (11, 8, 3, 1064): 4114}
LAYER_CASES = [((2, 3, 1, 36), 20, 9), ((2, 1, 3, 40), 20, 64)]  # (layout, K, C): the encoder's two input widths


def case_id(c):
    return "%d-%d-%d-%d-K%d-%s" % (c[0] + (c[1], c[2]))


def neighbour_lists(B, N, K, kind, rs):
    """(B, N, K) int32."""
    def perm_row(k):
        return np.concatenate([rs.permutation(N) for _ in range(-(-k // N))])[:k]
    if kind == "perm":
        idx = np.stack([np.stack([perm_row(K) for _ in range(N)]) for _ in range(B)])
    elif kind == "hubs":
        idx = np.stack([np.stack([np.r_[0, N - 1, perm_row(K - 2)] for _ in range(N)]) for _ in range(B)])
    elif kind == "repeats":
        def row():
            a = perm_row(K // 2)
            return np.r_[a, a[rs.permutation(K // 2)]]
        idx = np.stack([np.stack([row() for _ in range(N)]) for _ in range(B)])
    else:
        raise ValueError(kind)
    return torch.from_numpy(idx.astype(np.int32))


def _seed(lay, K, kind):
    return 7919 * lay[3] + 131 * lay[0] + 17 * lay[1] + 5 * lay[2] + 1000003 * K + {"perm": 0, "hubs": 1, "repeats": 2}[kind]


def _signed(g, n, lo, hi, every):
    """n values of magnitude in [lo, hi], negative at every `every`-th index + 1."""
    return (lo + (hi - lo) * torch.rand(n, generator=g)) * torch.where(torch.arange(n) % every == 1, -1.0, 1.0)


@functools.lru_cache(maxsize=None)
def case(lay, K, kind):
    """Host inputs and the float64 forward of a case, built once and shared.  Nothing here looks at a device."""
    from r3dfsseg_amd.ops import SegLayout
    seg = SegLayout(*lay)
    B, N, M = seg.B, seg.N, seg.M
    g = torch.Generator().manual_seed(_seed(lay, K, kind))
    rs = np.random.RandomState(_seed(lay, K, kind) % (2 ** 31))
    sig = (0.5 + 1.5 * torch.rand(64, generator=g)) / 2 ** 0.5
    PQ = torch.randn(M, 128, generator=g) * torch.cat((sig, sig))
    PQ[:, 64:] += 2 * torch.rand(64, generator=g) - 1
    famP, famQ = torch.randn(M, generator=g) / 2 ** 0.5, torch.randn(M, generator=g) / 2 ** 0.5
    for c, m in zip(FAMILY, FAMILY_MEAN):
        PQ[:, c], PQ[:, 64 + c] = famP, famQ + m
    PQ[:, 0], PQ[:, 64] = 0.75, 0.75
    idx = neighbour_lists(B, N, K, kind, rs)
    W2 = torch.randn(64, 64, generator=g) / 8
    gamma1, gamma2 = _signed(g, 64, 0.5, 1.5, 3), _signed(g, 64, 0.5, 1.5, 4)
    beta1, beta2 = _signed(g, 64, 0.1, 0.5, 2), _signed(g, 64, 0.0, 0.5, 5)
    counts = R.seg_counts(seg, K)
    st = R.stats1(PQ, idx, seg)
    bn1 = R.bnvec_of(R.fold(st["sums"], counts, gamma1, beta1, EPS)).float()
    fw = R.fwd(PQ, idx, bn1, W2, seg, keep_edges=False)
    bn2 = R.bnvec_of(R.fold(fw["sums2"], counts, gamma2, beta2, EPS)).float()
    sel = R.select(fw["zmax"], fw["zmin"], fw["argmax"], fw["argmin"], bn2, seg)
    zwin32 = sel["zwin"].float()
    # a winner closer than MARGIN to the kink of LeakyReLU-2 gets no gradient: whichever side a kernel puts it on, nothing
    # changes (decided on the reference alone; the share is capped like the other exemptions)
    near2 = R.u2_margin(zwin32, bn2, seg) < MARGIN
    dout = torch.randn(M, 64, generator=g)
    dout[near2] = 0.0
    exQ, exP = R.kink_edges(PQ, idx, bn1, seg, MARGIN)
    shares = dict(gap=float(((fw["gap_max"] < GAP) | (fw["gap_min"] < GAP)).float().mean()), u2=float(near2.float().mean()),
                  dQ=float(exQ.float().mean()), dP=float(exP.float().mean()))
    return dict(seg=seg, K=K, kind=kind, PQ=PQ, idx=idx, W2=W2, gamma1=gamma1, beta1=beta1, gamma2=gamma2, beta2=beta2,
                counts=counts, st=st, bn1=bn1, fw=fw, bn2=bn2, sel=sel, zwin32=zwin32, dout=dout, exQ=exQ, exP=exP, shares=shares)


def backward(c, dtype=R.F64):
    """The backward of a case on the INJECTED inputs: the reference's argmax, zwin and bn2_sums (fp32, as the device gets
    them)."""
    return R.bwd(c["PQ"], c["idx"], c["bn1"], c["bn2"], c["W2"], c["dout"], c["sel"]["win"], c["seg"], zwin=c["zwin32"],
                 bn2_sums=bn2_sums32(c), dtype=dtype)


def bn2_sums32(c):
    """(sum dy2, sum dy2 zhat2) per segment from the point-level winners in float64, rounded to fp32."""
    if "bn2_sums32" not in c:
        seg, bn2 = c["seg"], c["bn2"].double()
        rs = R.cloud_segments(seg).repeat_interleave(seg.N)
        z = c["zwin32"].double()
        dy = c["dout"].double() * R.act_slope(bn2[rs, 0] * z + bn2[rs, 1], 2)
        zh = (z - bn2[rs, 2]) * bn2[rs, 3]
        c["bn2_sums32"] = torch.stack([torch.stack((dy[r0:r1].sum(0), (dy * zh)[r0:r1].sum(0))) for r0, r1 in R.seg_slices(seg)]).float()
    return c["bn2_sums32"]


# ----------------------------------------------------------------------------------------------------------------------
# the layer, chained (x -> PQ -> ... -> gradients): the reference's own formulation maps to it through
# W1 = [Wa | Wb], PQ = x [Wa | Wb - Wa]^T
# ----------------------------------------------------------------------------------------------------------------------
def layer_inputs(lay, K, C, seed):
    from r3dfsseg_amd.ops import SegLayout
    seg = SegLayout(*lay)
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    return dict(seg=seg, K=K, C=C, x=torch.randn(seg.M, C, generator=g), idx=neighbour_lists(seg.B, seg.N, K, "perm", rs),
                W1=torch.randn(64, 2 * C, generator=g) * 0.4, W2=torch.randn(64, 64, generator=g) * 0.2,
                g1=_signed(g, 64, 0.3, 1.5, 3), b1=_signed(g, 64, 0.0, 0.3, 2), g2=_signed(g, 64, 0.3, 1.5, 4),
                b2=_signed(g, 64, 0.0, 0.3, 5), dout=torch.randn(seg.M, 64, generator=g))


def layer_ref(c, dtype=R.F64):
    """-> dict: out, dW1 (64, 2 C), dW2, dg1, db1, dg2, db2, dx; every stage from the previous one in `dtype`."""
    seg, K, C = c["seg"], c["K"], c["C"]
    x, W1 = c["x"].to(dtype), c["W1"].to(dtype)
    Wpq = torch.cat((W1[:, :C], W1[:, C:] - W1[:, :C]), 0)
    PQ = x @ Wpq.t()
    counts = R.seg_counts(seg, K)
    st = R.stats1(PQ, c["idx"], seg, dtype)
    bn1 = R.bnvec_of(R.fold(st["sums"], counts, c["g1"], c["b1"], EPS)).to(dtype)
    fw = R.fwd(PQ, c["idx"], bn1, c["W2"], seg, gamma2=c["g2"], beta2=c["b2"], eps=EPS, dtype=dtype, keep_edges=False)
    bw = R.bwd(PQ, c["idx"], bn1, fw["bn2"], c["W2"], c["dout"], fw["win"], seg, dtype=dtype)
    dPQ = torch.cat((bw["dP"], bw["dQ"]), 1)
    dWpq = dPQ.t() @ x
    return dict(out=fw["out"], dW1=torch.cat((dWpq[:64] - dWpq[64:], dWpq[64:]), 1), dW2=bw["dW2"], dx=dPQ @ Wpq,
                dg1=bw["bn1_sums"][:, 1].sum(0), db1=bw["bn1_sums"][:, 0].sum(0), dg2=bw["bn2_sums"][:, 1].sum(0),
                db2=bw["bn2_sums"][:, 0].sum(0))
