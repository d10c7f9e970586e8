"""The float64 references of tests/bn_ref.py against torch.nn.BatchNorm1d(...).double() in train mode, on the CPU: the
reference runs ONE SEGMENT AFTER THE OTHER through the module and autograd -- the schedule the segmented kernels
restate in one launch --, running statistics and num_batches_tracked included.  Bar: 1e-12 of the largest entry, the
tightest float64 allows on these sizes (measured: at most 1.5e-15).  What tests/test_gpu_bn_train.py compares the
kernels with is thereby nn.BatchNorm's own arithmetic."""
import pytest
import torch

import bn_ref as R
from r3dfsseg_amd.ops import SegLayout

BAR = 1e-12
EPS, MOM = 1e-5, 0.1
LAYOUTS = [(3, 3, 1, 10), (5, 2, 0, 7), (2, 1, 3, 5)]


def _close(got, want, what):
    e = R.rel(got, want)
    assert e <= BAR, (what, e)


def _inputs(seg, K, C, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(seg.M, K, generator=g, dtype=R.F64) + 0.3
    W = torch.randn(C, K, generator=g, dtype=R.F64) / K ** 0.5
    gamma = (torch.rand(C, generator=g, dtype=R.F64) + 0.5) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    beta = torch.rand(C, generator=g, dtype=R.F64) - 0.5
    bias = torch.randn(C, generator=g, dtype=R.F64)
    dY = torch.randn(seg.M, C, generator=g, dtype=R.F64)
    return X, W, gamma, beta, bias, dY


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("E,S,Q,N", LAYOUTS)
def test_layer_is_batchnorm1d_segment_after_segment(E, S, Q, N, act):
    seg = SegLayout(E, S, Q, N)
    K, C = 6, 9
    X, W, gamma, beta, bias, dY = _inputs(seg, K, C, 10 * E + act)
    # reference: the module itself, one call per segment, in segment order
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).double().train()
    bn.weight.data, bn.bias.data = gamma.clone(), beta.clone()
    bn.running_mean.data = torch.linspace(-1, 1, C, dtype=R.F64)
    bn.running_var.data = torch.linspace(0.5, 2, C, dtype=R.F64)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    Xr, Wr, br = X.clone().requires_grad_(), W.clone().requires_grad_(), bias.clone().requires_grad_()
    ys, us = [], []
    for r0, r1 in R.seg_slices(seg):
        u = bn(Xr[r0:r1] @ Wr.t() + br)
        us.append(u.detach())
        ys.append(R.act_fwd(u, act))
    y = torch.cat(ys)
    (y * dY).sum().backward()
    assert int(bn.num_batches_tracked) == seg.n_seg == len(R.seg_counts(seg))
    # bn_ref
    fw = R.layer_fwd(X, W, gamma, beta, act, seg, EPS)
    bw = R.layer_bwd(fw, dY)
    _close(fw["u"], torch.cat(us), "u")
    _close(fw["y"], y.detach(), "y")
    _close(bw["dW"], Wr.grad, "dW")
    _close(bw["dX"], Xr.grad, "dX")
    _close(bw["dgamma"], bn.weight.grad, "dgamma")
    _close(bw["dbeta"], bn.bias.grad, "dbeta")
    assert br.grad.abs().max() <= 1e-12 * dY.abs().sum(0).max()  # a bias in front of batch statistics: gradient 0
    rm, rv = R.running(rm0, rv0, fw["records"], MOM, bias=bias)
    _close(rm, bn.running_mean, "running_mean")
    _close(rv, bn.running_var, "running_var")
    # the stages one by one, on the layer's z
    z = fw["z"]
    sums, terms = R.colsums(z, seg, 0)
    f = R.fold(sums, R.seg_counts(seg), gamma, beta, EPS)
    for s, (r0, r1) in enumerate(R.seg_slices(seg)):
        _close(f["mean"][s], z[r0:r1].mean(0), "mean")
        _close(f["var"][s], z[r0:r1].var(0, unbiased=False), "var")
        _close(f["unbiased"][s], z[r0:r1].var(0, unbiased=True), "unbiased")
        _close(f["invstd"][s], 1 / torch.sqrt(z[r0:r1].var(0, unbiased=False) + EPS), "invstd")
        assert (terms[s, 0] >= sums[s, 0].abs()).all() and torch.equal(terms[s, 1], sums[s, 1])
    ya, mag = R.affine_act(z, seg, R.bnvec_of(f), act)
    _close(ya, y.detach(), "affine_act")
    assert (mag >= fw["u"].abs() * (1 - 1e-15)).all()
    # the backward's two stages against autograd through the normalisation alone
    zr = z.clone().requires_grad_()
    bn2 = torch.nn.BatchNorm1d(C, eps=EPS).double().train()
    bn2.weight.data, bn2.bias.data = gamma.clone(), beta.clone()
    (torch.cat([R.act_fwd(bn2(zr[r0:r1]), act) for r0, r1 in R.seg_slices(seg)]) * dY).sum().backward()
    s1, _ = R.colsums(z, seg, 1, DY=dY, bnvec=fw["bnvec"], act=act)
    dz, _ = R.bwd_apply(z, dY, seg, fw["bnvec"], act, s1, R.seg_counts(seg))
    _close(dz, zr.grad, "dz")
    _close(s1[:, 0].sum(0), bn2.bias.grad, "sum du")
    _close(s1[:, 1].sum(0), bn2.weight.grad, "sum du zhat")


def test_fold_edges_count_one_clamp_and_edge_counts():
    """count 1: mean = x, var = 0, no Bessel factor; sums whose variance comes out negative are clamped; a count other
    than the row count (EdgeConv: K edges per row) divides as given."""
    C = 4
    gamma, beta = torch.tensor([1.0, -2.0, 0.5, 1.5], dtype=R.F64), torch.tensor([0.1, 0.2, -0.3, 0.0], dtype=R.F64)
    x = torch.tensor([[3.0, -1.0, 0.0, 2.5]], dtype=R.F64)
    seg = SegLayout(1, 1, 0, 1)
    sums, _ = R.colsums(x, seg, 0)
    f = R.fold(sums, R.seg_counts(seg), gamma, beta, EPS)
    assert torch.equal(f["mean"][0], x[0]) and (f["var"] == 0).all() and (f["unbiased"] == 0).all()
    _close(f["invstd"][0], torch.full((C,), EPS ** -0.5, dtype=R.F64), "invstd at var 0")
    _close(f["scale"][0] * x[0] + f["shift"][0], beta, "y = beta at var 0")
    neg = torch.tensor([[[10.0, 10.0, 10.0, 10.0], [24.9, 25.0, 25.1, 30.0]]], dtype=R.F64)  # n = 4: mean 2.5, E x^2 - 6.25
    f = R.fold(neg, [4.0], gamma, beta, EPS)
    assert f["var"][0, 0] == 0 and f["var"][0, 1] == 0 and f["var"][0, 2] > 0
    seg = SegLayout(2, 1, 2, 3)
    assert R.seg_counts(seg, per_row=20) == [60.0, 120.0, 60.0, 120.0]
    assert R.seg_slices(seg) == [(0, 3), (3, 9), (9, 12), (12, 18)]
    assert R.row_segments(seg).tolist() == [0] * 3 + [1] * 6 + [2] * 3 + [3] * 6
    assert R.seg_slices(SegLayout(3, 2, 0, 2)) == [(0, 4), (4, 8), (8, 12)]


@pytest.mark.parametrize("E,S,Q,N,C", [(3, 3, 1, 100, 64), (1, 19, 1, 64, 1024), (1, 1, 0, 513, 96), (1, 1, 0, 31, 16)])
def test_fp32_partition_sums_are_the_float64_sums_within_the_partition_bound(E, S, Q, N, C):
    """colsums_f32 (the e32 of the GPU tests) restates colsums in fp32 in the kernels' partition: at most 128 fp32
    additions per wave partial, 3 between the waves, one rounding of each term and of the result."""
    seg = SegLayout(E, S, Q, N)
    g = torch.Generator().manual_seed(C + N)
    X = torch.randn(seg.M, C, generator=g) + 2.0
    DY = torch.randn(seg.M, C, generator=g)
    bnvec = torch.randn(seg.n_seg, 4, C, generator=g)
    X = R.clear_kink(X, seg, bnvec, 1e-3)  # (no pre-activation within rounding of the kink: the slopes are the same)
    assert R.kink_margin(X, seg, bnvec) >= 1e-3
    for mode, act in ((0, 0), (1, 0), (1, 2)):
        s64, terms = R.colsums(X, seg, mode, DY=DY, bnvec=bnvec, act=act)
        s32 = R.colsums_f32(X, seg, mode, DY=DY, bnvec=bnvec, act=act)
        e = float(((s32.to(R.F64) - s64).abs() / terms).max())
        assert 0 < e <= (128 + 3 + 4) * R.ULP, (mode, act, e)
    assert [R.ts_chunks(r, C) for r in (1, 31, 65, 513, 300, 100, 1216)] == [1, 1, 1, 6, 4, 1, 19]
