"""Float64 restatement of the two GEMM-shaped entry points that decide no index, for tests/test_gpu_gemm_kernels.py;
tests/test_gemm_ref_host.py holds it to torch without a GPU.

  point-wise (csrc/gemm.hip, csrc/gemm_bx3.hip):   Out = act(scale * X W^T + shift) (+ Out)
  weight gradient (csrc/train_ops.hip, gemm_bx3):  out = alpha A^T B (+ out)

``*32``: the same in fp32 as ONE running sum in k (row) order, product and sum rounded separately -- the ``e32`` figure the
GPU tests print beside every device figure.  ``*_bound``: the denominator of the error figure, the size of what was summed:
|scale| sum_k |x||w| + |shift| (+ |pre|), |alpha| sum_m |a||b| (+ |pre|)."""
import numpy as np
import torch

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def _np(t, dtype):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).astype(dtype)


def _act(v, act):
    if act == ACT_RELU:
        return np.maximum(v, 0)
    if act == ACT_LRELU:
        return np.where(v > 0, v, v.dtype.type(0.2) * v)
    assert act == ACT_NONE, act
    return v


def _epilogue(z, scale, shift, act, pre):
    if scale is not None:
        z = z * scale[None, :]
    if shift is not None:
        z = z + shift[None, :]
    z = _act(z, act)
    return z if pre is None else pre + z


def pointwise(X, W, scale=None, shift=None, act=0, pre=None):
    """X (M, K), W (Co, K), scale / shift (Co) or None, pre (M, Co) or None (accumulate) -> float64 (M, Co) ndarray."""
    X, W, scale, shift, pre = (_np(t, np.float64) for t in (X, W, scale, shift, pre))
    return _epilogue(X @ W.T, scale, shift, act, pre)


def pointwise32(X, W, scale=None, shift=None, act=0, pre=None):
    """The same in fp32: z a running sum over k = 0, 1, ..; scale * z, + shift, act, + pre each rounded once."""
    X, W, scale, shift, pre = (_np(t, np.float32) for t in (X, W, scale, shift, pre))
    z = np.zeros((X.shape[0], W.shape[0]), np.float32)
    for k in range(X.shape[1]):
        z += X[:, k:k + 1] * W[None, :, k]
    out = _epilogue(z, scale, shift, act, pre)
    assert out.dtype == np.float32
    return out


def pointwise_bound(X, W, scale=None, shift=None, pre=None):
    X, W, scale, shift, pre = (_np(t, np.float64) for t in (X, W, scale, shift, pre))
    b = np.abs(X) @ np.abs(W).T
    if scale is not None:
        b = b * np.abs(scale)[None, :]
    if shift is not None:
        b = b + np.abs(shift)[None, :]
    return b if pre is None else b + np.abs(pre)


def gemm_tn(A, B, alpha=1.0, pre=None):
    """A (M, Ca), B (M, Cb), pre (Ca, Cb) or None (accumulate) -> float64 (Ca, Cb) ndarray; alpha as the fp32 the ABI takes."""
    A, B, pre = (_np(t, np.float64) for t in (A, B, pre))
    out = float(np.float32(alpha)) * (A.T @ B)
    return out if pre is None else pre + out


def gemm_tn32(A, B, alpha=1.0, pre=None):
    """The same in fp32: a running sum over the rows m = 0, 1, ..; alpha * sum and + pre each rounded once."""
    A, B, pre = (_np(t, np.float32) for t in (A, B, pre))
    z = np.zeros((A.shape[1], B.shape[1]), np.float32)
    for m in range(A.shape[0]):
        z += A[m][:, None] * B[m][None, :]
    out = np.float32(alpha) * z
    out = out if pre is None else pre + out
    assert out.dtype == np.float32
    return out


def gemm_tn_bound(A, B, alpha=1.0, pre=None):
    A, B, pre = (_np(t, np.float64) for t in (A, B, pre))
    b = abs(float(np.float32(alpha))) * (np.abs(A).T @ np.abs(B))
    return b if pre is None else b + np.abs(pre)


def figure(got, ref64, bound):
    """max |got - ref64| / bound over the tensor.  Where the bound is 0 (a zero scale without a shift, a zero column) every
    term of the sum is 0 and the result must be 0 exactly: asserted here, and left out of the maximum."""
    got = _np(got, np.float64)
    assert got.shape == ref64.shape == bound.shape, (got.shape, ref64.shape, bound.shape)
    assert np.isfinite(got).all(), "a result is not finite"
    zero = bound == 0
    assert (got[zero] == 0).all() and (ref64[zero] == 0).all(), "a sum of zeros is not zero"
    if zero.all():
        return 0.0
    return float((np.abs(got - ref64)[~zero] / bound[~zero]).max())
