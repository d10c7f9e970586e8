"""Float64 reference of the attention training kernels (csrc/attention.hip), for tests/test_gpu_attention_kernels.py and
tests/test_gpu_output_dim.py; tests/test_attn_ref_host.py holds it to torch autograd, to the oracle and to the reference's
golden vectors without a GPU.

``dtype``: float64 is the reference, float32 is the same dense formula in the kernels' precision on the CPU (the ``e32``
the GPU tests print beside each measured error)."""
import numpy as np
import torch

M32 = 0xFFFFFFFF

# (seed, p_drop, B, N) of the dropout-edge cases of tests/test_gpu_attention_kernels.py (found by a search over seeds 1, 2, ..; proven in
# tests/test_attn_ref_host.py)
ALL_DROPPED = (2, 0.9, 3, 33)    # rows (0, 23), (1, 15), (1, 20), (2, 8), (2, 21) keep no key at all
ALL_DROPPED_ROWS = [(0, 23), (1, 15), (1, 20), (2, 8), (2, 21)]
TILE_DROPPED = (1, 0.9, 2, 65)   # row (1, 34) keeps no key of 32 .. 63, but keys of 0 .. 31 and key 64
TILE_DROPPED_ROW = (1, 34)


def threshold(p_drop):
    """The kernels' `(unsigned)(p_drop * 4294967296.0)` for a float p_drop."""
    return int(float(np.float32(p_drop)) * 4294967296.0)


def keep_hash(seed, row, key):
    """csrc/attention.hip::attn_keep's hash of one (row, key) in integer arithmetic modulo 2^32; row and key may be int64
    tensors that broadcast."""
    x = ((row * 0x9E3779B1) & M32) ^ ((key * 0x85EBCA77) & M32) ^ (seed & M32)
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    x = x ^ (x >> 16)
    return x


def keep_mask(B, N, seed, p_drop, seed_dev=0, group=0):
    """csrc/attention.hip::attn_keep for every (cloud, query, key) -> bool (B, N, N), True = kept.
    Effective seed seed + seed_dev + 2 (b // group) modulo 2^32 (group = 0: seed + seed_dev); hash row
    (b % group) N + query when group > 0, else b N + query."""
    b = torch.arange(B, dtype=torch.int64).view(B, 1, 1)
    query = torch.arange(N, dtype=torch.int64).view(1, N, 1)
    key = torch.arange(N, dtype=torch.int64).view(1, 1, N)
    if group > 0:
        eff = (seed + seed_dev + 2 * torch.div(b, group, rounding_mode="floor")) & M32
        row = ((b % group) * N + query) & M32
    else:
        eff = torch.full((B, 1, 1), (seed + seed_dev) & M32, dtype=torch.int64)
        row = (b * N + query) & M32
    return keep_hash(eff, row, key) >= threshold(p_drop)


def attention(qkv, B, N, D, dO, keep=None, p_drop=0.0, q_scale=1.0, dtype=torch.float64):
    """Restatement of models/attention.py:43-46 (q arrives scaled) and its gradient w.r.t. q | k | v, dense, in `dtype`.
    qkv (B N, >= 3 D) holds q | k | v at columns 0 | D | 2 D, dO (B N, D); keep: bool (B, N, N) or None.
    -> out (B N, D), lse (B N) = logsumexp of the scores, rowdot (B N) = <dO, out>, dqkv (B N, 3 D) = dq q_scale | dk | dv."""
    q, k, v = (qkv[:, D * i:D * (i + 1)].detach().cpu().to(dtype).reshape(B, N, D) for i in range(3))
    s = q @ k.transpose(1, 2)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        one = torch.tensor(1.0, dtype=dtype)
        sc = keep.to(dtype) * (one / (one - torch.tensor(float(np.float32(p_drop)), dtype=dtype)))
    else:
        sc = 1.0
    Pd = P * sc
    out = Pd @ v
    g = dO.detach().cpu().to(dtype).reshape(B, N, D)
    rowdot = (g * out).sum(-1)
    dV = Pd.transpose(1, 2) @ g
    dP = (g @ v.transpose(1, 2)) * sc
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    dq = (dS @ k) * torch.tensor(float(q_scale), dtype=dtype)
    dqkv = torch.cat((dq, dS.transpose(1, 2) @ q, dV), -1)
    return out.reshape(B * N, D), lse.reshape(B * N), rowdot.reshape(B * N), dqkv.reshape(B * N, 3 * D)


def rel(got, want):
    """max |got - want| / max |want| (both cast to float64 on the CPU)."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return ((got - want).abs().max() / want.abs().max()).item()
