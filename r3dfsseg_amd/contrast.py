"""Per-way contrastive loss (reference models/mpti.py:226-313) as plain halves around r3d_contrast_fwd / r3d_contrast_bwd
(contrast_forward / contrast_backward, on a batch of E episodes as in train_ops.py), their autograd adapter for one
episode (ContrastFn, behind per_way_contrast_loss), and the training-only debug metrics (mpti.py:515-568)."""
from collections import namedtuple

import torch

from . import _lib, ops
from .ops import _p, _st

ContrastSaved = namedtuple("ContrastSaved", "model ws words E ep_rows")


def contrast_forward(model, sfeat, W, b, support_y, support_flag, E=1, ep_rows=0):
    """sfeat: support rows of episode 0 (episode e's start e * ep_rows rows further on) -> (loss (E,), saved)."""
    lib = _lib.load()
    S, N, D = model.n_way * model.k_shot, model.n_points, model.feat_dim
    dev = sfeat.device
    words = lib.r3d_contrast_ws_words(model.n_way, model.k_shot, N)
    ws = torch.empty(E, words, device=dev, dtype=torch.float32)
    loss = torch.empty(E, device=dev, dtype=torch.float32)
    sy = support_y.reshape(E, S, N).to(torch.int32).contiguous()
    sf = support_flag.reshape(E, S).to(torch.int32).contiguous()
    Wc, bc = W.detach().contiguous(), b.detach().contiguous()
    _lib.check(lib.r3d_contrast_fwd_batched(E, _p(sfeat), sfeat.stride(0), ep_rows, D, _p(sy), _p(sf), model.n_way,
                                            model.k_shot, N, _p(Wc), _p(bc), 0.1, _p(loss), _p(ws), words, words, _st()))
    return loss, ContrastSaved(model, ws, words, E, ep_rows)


def contrast_backward(saved, gscale, rows):
    """-> (dfeat (rows, D), dW, db) of gscale * sum_e loss[e].  `rows` is the caller's: the support rows alone (one
    episode under autograd) or all rows of the batch's feature matrix, zero wherever no support row of an episode lies;
    dW, db are summed over the batch."""
    model, ws, words, E, ep_rows = saved
    lib = _lib.load()
    dev = ws.device
    D, N = model.feat_dim, model.n_points
    gs = gscale.reshape(-1)[:1].to(torch.float32).contiguous()
    dfeat = torch.zeros(rows, D, device=dev, dtype=torch.float32)
    dW = torch.empty(128, D, device=dev, dtype=torch.float32)
    db = torch.empty(128, device=dev, dtype=torch.float32)
    _lib.check(lib.r3d_contrast_bwd_batched(E, D, model.n_way, model.k_shot, N, _p(gs), _p(dfeat), D, ep_rows, _p(dW), _p(db),
                                            _p(ws), words, _st()))
    return dfeat, dW, db


class ContrastFn(torch.autograd.Function):
    """The autograd adapter of contrast_forward / contrast_backward for ONE episode: (sfeat, W, b) -> loss (0-d)."""

    @staticmethod
    def forward(ctx, sfeat, W, b, model, support_y, support_flag):
        loss, ctx.saved = contrast_forward(model, sfeat, W, b, support_y, support_flag)
        ctx.rows = sfeat.shape[0]
        return loss[0]

    @staticmethod
    def backward(ctx, gloss):
        return contrast_backward(ctx.saved, gloss, ctx.rows) + (None, None, None)


def per_way_contrast_loss(model, sfeat, support_y, support_flag):
    return ContrastFn.apply(sfeat, model.proj.weight, model.proj.bias, model, support_y, support_flag)


def train_debug_metrics(model, hb, pred, support_y, gt_support_y, query_y, gt_query_y, logger=None):
    """(query_acc_LP, query_acc_original, clean_ratio_LP_avg, clean_ratio_original_avg) of every episode in the head
    buffers `hb`, as an (E, 4) device tensor; `pred` (E, n_q, N) int32 is the head's arg-max (head_train.lp_forward)."""
    lib = _lib.load()
    N = model.n_points
    S = model.n_way * model.k_shot
    n_ep = hb.E
    out = torch.empty(n_ep, 4, device=hb.Z.device, dtype=torch.float32)
    n_qpts = pred.numel() // n_ep
    qy = query_y.to(torch.int64).contiguous()
    gq = (gt_query_y if gt_query_y is not None else query_y).to(torch.int64).contiguous()
    gs = (gt_support_y if gt_support_y is not None else support_y).reshape(-1).to(torch.int32).contiguous()
    _lib.check(lib.r3d_train_metrics_batched(n_ep, _p(pred), _p(qy), _p(gq), n_qpts, _p(hb.Z), hb.n_cap, _p(hb.desc), ops.HD_WORDS,
                                             _p(hb.proto_ws), hb.proto_stride, _p(hb.assign), 2 * S * N, _p(gs), model.n_way,
                                             model.k_shot, N, _p(out), _st()))
    if logger is not None:  # the reference prints these every step (mpti.py:546,568): a host sync, as there
        v = out[0].tolist()
        logger.cprint('after label propagation: QUERY prediction acc: {:.3f}, original_acc: {:.3f}'.format(v[0], v[1]))
        logger.cprint('after label propagation: clean_ratio_LP: {:.3f}, clean_ratio_original: {:.3f}'.format(v[2], v[3]))
    return out
