"""A from-scratch torch restatement of ProtoNet_Contrast's head (models/protonet.py:878-940: getMaskedFeatures,
getPrototype(clean_flag=...), calculateSimilarity), for the tests of r3d_protonet_head_keep_batched.  float64 throughout
unless told otherwise, channel-major as the reference: support_feat (n_way, k_shot, D, N), query_feat (n_q, D, N),
support_y (n_way, k_shot, N) of 0 / 1, keep (n_way, k_shot) of 0 / 1 or None (every shot kept)."""
import torch


def masked_pool(feat, mask):
    """sum(feat * mask) / (mask.sum() + 1e-5) over the points -> (n_way, k_shot, D)."""
    mask = mask.to(feat.dtype).unsqueeze(2)
    return (feat * mask).sum(3) / (mask.sum(3) + 1e-5)


def keep_prototypes(fg, bg, keep=None):
    """fg, bg (n_way, k_shot, D) pooled features -> (n_way + 1, D), background first.  A way's foreground prototype is the
    sum over its KEPT shots over the NUMBER kept; the background prototype the sum over ALL shots over n_way * k_shot."""
    n_way, k_shot, _ = fg.shape
    keep = torch.ones(n_way, k_shot, dtype=fg.dtype) if keep is None else keep.reshape(n_way, k_shot).to(fg.dtype)
    if not bool((keep.sum(1) > 0).all()):
        raise ValueError("a way without a kept shot has no prototype")
    fgp = (fg * keep.unsqueeze(-1)).sum(1) / keep.sum(1, keepdim=True)
    bgp = bg.sum((0, 1)) / (n_way * k_shot)
    return torch.cat((bgp[None], fgp), 0)


def similarity(query_feat, protos, method, scaler=10.0):
    """(n_q, D, N) against (C, D) -> (n_q, C, N): cosine * scaler (the norms' product clamped at 1e-8) or minus the squared
    euclidean distance with torch 1.8's pairwise_distance eps: ||q - p + 1e-6||^2."""
    q = query_feat.unsqueeze(1)                    # (n_q, 1, D, N)
    p = protos[None, :, :, None]                   # (1, C, D, 1)
    if method == "cosine":
        den = (q.norm(dim=2) * p.norm(dim=2)).clamp(min=1e-8)
        return (q * p).sum(2) / den * scaler
    if method == "euclidean":
        return -((q - p + 1e-6) ** 2).sum(2)
    raise NotImplementedError(method)


def head(support_feat, support_y, query_feat, keep, method, dtype=torch.float64):
    sf, qf = support_feat.to(dtype), query_feat.to(dtype)
    fg = masked_pool(sf, support_y == 1)
    bg = masked_pool(sf, support_y == 0)
    return similarity(qf, keep_prototypes(fg, bg, keep), method)
