"""Restatement of the ProtoNet head (models/protonet.py:295-349) in plain torch, differentiable by autograd: the checker of
tests/test_protonet_train_golden.py (which holds it to the reference's recorded loss and gradients) and of
tests/test_gpu_protonet_train.py (which holds the HIP kernels to it in float64).  Not a test module.

    fg_s = sum_p m_sp f_sp / (n_s + 1e-5)          bg_s = sum_p (1 - m_sp) f_sp / (N - n_s + 1e-5)      s = way * k_shot + k
    P_0 = sum_s bg_s / (n_way k_shot)              P_{w+1} = sum_k fg_{w,k} / k_shot
    cosine:    Z_pc = scaler <q_p, P_c> / max(|q_p| |P_c|, 1e-8)     (torch 1.8 clamps the PRODUCT of the norms)
    euclidean: Z_pc = -sum_d (q_pd - P_cd + 1e-6)^2                  (torch 1.8's pairwise_distance: norm(x1 - x2 + eps))
"""
import torch
import torch.nn.functional as F


def prototypes(sfeat, support_y, n_way, k_shot, N):
    """sfeat (S*N, D), support_y (S, N) in {0, 1} -> (n_way + 1, D), background first."""
    S = n_way * k_shot
    f = sfeat.reshape(S, N, -1)
    m = support_y.reshape(S, N, 1).to(f.dtype)
    n = m.sum(1)
    fg = (f * m).sum(1) / (n + 1e-5)
    bg = (f * (1 - m)).sum(1) / ((N - n) + 1e-5)
    return torch.cat((bg.sum(0, keepdim=True) / S, fg.reshape(n_way, k_shot, -1).sum(1) / k_shot), 0)


def similarity(qfeat, P, method, scaler=10.0):
    """qfeat (n_pts, D), P (C, D) -> Z (n_pts, C)."""
    if method == "cosine":
        den = (qfeat.norm(dim=1, keepdim=True) * P.norm(dim=1)[None]).clamp(min=1e-8)
        return scaler * (qfeat @ P.t()) / den
    if method == "euclidean":
        return -((qfeat[:, None, :] - P[None] + 1e-6) ** 2).sum(-1)
    raise NotImplementedError('Error! Distance computation method (%s) is unknown!' % method)


def head(sfeat, qfeat, support_y, n_way, k_shot, N, method, scaler=10.0):
    return similarity(qfeat, prototypes(sfeat, support_y, n_way, k_shot, N), method, scaler)


def logits_and_loss(Z, query_y):
    """Z (n_q*N, C), query_y (n_q, N) int64 -> logits (n_q, C, N), mean cross entropy (protonet.py:262-275)."""
    n_q, N = query_y.shape
    logits = Z.reshape(n_q, N, -1).permute(0, 2, 1)
    return logits, F.cross_entropy(logits, query_y)


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm().clamp(min=1e-300))
