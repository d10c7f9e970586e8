"""Float64 reference of the inference EdgeConv kernel (csrc/edgeconv.hip: r3d_edgeconv_kernel behind r3d_edgeconv_fwd), restated
from the operands as the C entry point takes them, and the cases of tests/test_gpu_edge_fwd.py.
tests/test_edge_fwd_ref_host.py holds it to oracle.r3d_oracle (get_edge_feature + conv_block + max) without a GPU.

  h1(i, t)  = lrelu(P[idx[i][t]] + Q[i])                       PQ (B N, 128) = [P | Q], idx (B, N, K) local to the cloud
  v(i, t)   = lrelu(s2 * (W2 h1(i, t)) + t2)                   W2 (64, 64) [out][in], s2 / t2 (64)
  out[i]    = max_t v(i, t),  argmax[i] = the lowest slot t that attains it (torch.max)

Neighbour ids outside [0, N) are clamped, as include/r3d.h promises.

``bound`` (point, channel) = 16 * 2^-24 * max_t (|s2| * sum_k |W2||h1(i, t)| + |t2|): what two fp32 evaluations of v -- a
64-term sum, an affine map and a LeakyReLU each -- can differ by from their float64 values together (8 ulps of the summed
magnitude each).  A device winner is right when the float64 value at its slot is within ``bound`` of the float64 maximum;
where the float64 gap to the best OTHER neighbour exceeds ``bound`` that is the same as demanding the float64 arg-max."""
from collections import namedtuple

import numpy as np
import torch

EdgeCase = namedtuple("EdgeCase", "name B N K what")

KS = tuple(range(4, 33, 4))
CASES = ([EdgeCase("B3 N8 K%d" % k, 3, 8, k, "two units per cloud, three clouds; lists longer than the cloud repeat neighbours"
                   if k > 8 else "two units per cloud, three clouds") for k in KS]
         + [EdgeCase("B2 N132 K%d" % k, 2, 132, k, "33 units per cloud: a cloud boundary inside the walk, N no multiple of 8")
            for k in KS]
         + [EdgeCase("B1 N4 K4", 1, 4, 4, "one unit, one workgroup"),
            EdgeCase("B2 N2052 K4", 2, 2052, 4, "1026 units: above the 1024-workgroup cap every launch walks several units per "
                     "workgroup"),
            EdgeCase("B2 N2052 K32", 2, 2052, 32, "the same with the largest tile")])
NEAR_TIE_CAP = 0.01  # share of (point, channel) entries whose float64 gap to the best other neighbour is within `bound`


def lists(B, N, K, rs):
    """(B, N, K) int32 neighbour lists drawn WITHOUT replacement: whole random permutations of the cloud one after the other,
    cut at K -- distinct neighbours when K <= N, every neighbour at most ceil(K / N) times otherwise."""
    out = np.empty((B, N, K), np.int32)
    for b in range(B):
        for i in range(N):
            out[b, i] = np.concatenate([rs.permutation(N) for _ in range(-(-K // N))])[:K]
    return out


def make(case, seed=0):
    """-> dict of fp32 / int32 torch tensors on the CPU: PQ (B N, 128), idx (B, N, K), W2, s2 (some negative), t2."""
    B, N, K = case.B, case.N, case.K
    rs = np.random.RandomState(100003 * B + 101 * N + K + seed)
    s2 = (rs.randn(64) * 0.3 + 1.0).astype(np.float32)
    s2[::5] *= -1.0
    return dict(PQ=torch.from_numpy((rs.randn(B * N, 128) * 0.7).astype(np.float32)),
                idx=torch.from_numpy(lists(B, N, K, rs)),
                W2=torch.from_numpy((rs.randn(64, 64) / 8.0).astype(np.float32)),
                s2=torch.from_numpy(s2), t2=torch.from_numpy((rs.randn(64) * 0.3).astype(np.float32)))


def _lrelu(x):
    return torch.where(x > 0, x, x * 0.2)


def slots(PQ, idx, W2, s2, t2, dtype=torch.float64):
    """-> v (B N, K, 64): the activated second layer of every edge, and mag (B N, K, 64) = |s2| sum_k |W2||h1| + |t2|."""
    B, N, K = idx.shape
    PQ, W2, s2, t2 = (t.detach().cpu().to(dtype) for t in (PQ, W2, s2, t2))
    nb = idx.detach().cpu().long().clamp(0, N - 1) + (torch.arange(B) * N).view(B, 1, 1)  # global rows
    h1 = _lrelu(PQ[:, :64][nb.reshape(B * N, K)] + PQ[:, None, 64:])                      # (B N, K, 64)
    v = _lrelu(s2 * (h1 @ W2.t()) + t2)
    mag = s2.abs() * (h1.abs() @ W2.abs().t()) + t2.abs()
    return v, mag


def reference(PQ, idx, W2, s2, t2, dtype=torch.float64):
    """-> out (B N, 64), argmax (B N, 64) int64 (lowest slot), v, bound (B N, 64) in float64."""
    v, mag = slots(PQ, idx, W2, s2, t2, dtype)
    out, am = v.max(dim=1)
    # torch.max returns SOME maximal index on ties; the lowest one:
    am = (v == out.unsqueeze(1)).to(torch.int64).argmax(dim=1)
    return out, am, v, (16.0 * 2.0 ** -24) * mag.double().max(dim=1)[0]


def other_gap(v, idx, N):
    """(B N, 64) float64 gap between the maximum and the best slot that names ANOTHER neighbour than the winner's (inf when
    every slot names the winner's)."""
    B, _, K = idx.shape
    nb = idx.detach().cpu().long().clamp(0, N - 1).reshape(B * N, K)
    out, am = v.max(dim=1)
    win_nb = torch.gather(nb, 1, am)                                           # (B N, 64)
    same = nb.unsqueeze(-1) == win_nb.unsqueeze(1)                             # (B N, K, 64)
    rest = torch.where(same, torch.full_like(v, -float("inf")), v).max(dim=1)[0]
    return (out - rest).double()


def near_tie_share(v, idx, N, bound):
    return (other_gap(v, idx, N) <= bound).double().mean().item()


def winners_ok(v, am_dev, bound):
    """Every entry: the float64 value at the device's slot is within bound of the float64 maximum -> bool (B N, 64)."""
    at = torch.gather(v, 1, am_dev.long().unsqueeze(1)).squeeze(1)
    return at >= v.max(dim=1)[0] - bound


def lowest_slot_of_winner(v, idx, N):
    """(B N, 64) the lowest slot that names the float64 winner's neighbour."""
    B, _, K = idx.shape
    nb = idx.detach().cpu().long().clamp(0, N - 1).reshape(B * N, K)
    win_nb = torch.gather(nb, 1, v.max(dim=1)[1])
    return (nb.unsqueeze(-1) == win_nb.unsqueeze(1)).to(torch.int64).argmax(dim=1)
