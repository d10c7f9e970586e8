"""Training-mode forward of ProtoNet (reference models/protonet.py:245-275 under model.train()) and the autograd edge of its
head.  Compute lives in libr3d_hip.so (csrc/protonet_train.hip); this file orders launches."""
import torch

from . import _lib, ops, train_ops as T
from .ops import SegLayout, _p, _st


class ProtoHeadFn(torch.autograd.Function):
    """(sfeat, qfeat) -> cross-entropy loss of the prototype similarities; leaves logits / arg-max in model._train_logits /
    model._train_pred.  backward writes both feature gradients into ONE (S*N + n_q*N, D) matrix, support rows first -- the
    layout train_ops.EncoderTrainFn.backward consumes -- and returns its two row ranges."""

    @staticmethod
    def forward(ctx, sfeat, qfeat, model, support_y, query_y):
        N = model.n_points
        n_q = query_y.shape[-2]
        Z, ws = ops.protonet_head_train(sfeat, qfeat, support_y, model.n_way, model.k_shot, N, model.dist_method)
        labels = query_y.reshape(n_q, N).to(torch.int64).contiguous()
        logits, loss, pred = ops.logits_ce_from_rows(Z, n_q, N, model.n_way + 1, labels)
        ctx.model, ctx.Z, ctx.ws, ctx.labels, ctx.n_q = model, Z, ws, labels, n_q
        ctx.qfeat, ctx.support_y = qfeat, support_y
        model._train_logits, model._train_pred = logits, pred
        return loss

    @staticmethod
    def backward(ctx, gloss):
        model, Z, n_q = ctx.model, ctx.Z, ctx.n_q
        dev = Z.device
        N, D = model.n_points, model.feat_dim
        S = model.n_way * model.k_shot
        gs = gloss.reshape(-1)[:1].to(torch.float32).contiguous()
        zero = torch.zeros(1, device=dev, dtype=torch.int32)  # (no prototype rows in front of the query rows)
        G = torch.empty_like(Z)
        _lib.check(_lib.load().r3d_ce_grad_batched(1, _p(Z), _p(zero), 0, n_q * N, n_q * N, model.n_way + 1, _p(ctx.labels), _p(gs),
                                                   _p(G), _st()))
        dfeat = torch.empty((S + n_q) * N, D, device=dev, dtype=torch.float32)
        ops.protonet_head_bwd(ctx.qfeat, ctx.support_y, model.n_way, model.k_shot, N, model.dist_method, G, ctx.ws,
                              dfeat[:S * N], dfeat[S * N:])
        return dfeat[:S * N], dfeat[S * N:], None, None, None


def protonet_train_forward(model, support_x, support_y, query_x, query_y):
    """Returns the reference's pair (protonet.py:275): query_pred (n_q, n_way + 1, N) and the loss, which carries the graph."""
    S, N = model.n_way * model.k_shot, model.n_points
    seed = T.next_dropout_seed(model)
    sx = support_x.reshape(S, model.in_channels, N)
    # two getFeatures calls, each with its own BatchNorm batch statistics, support first (protonet.py:256-258), through one
    # launch sequence over the S + Q clouds
    seg = SegLayout(1, S, query_x.shape[0], N)
    sfeat, qfeat = T.get_features_train(model, ops.cat_clouds(sx, query_x, 0), seed, seg=seg)
    if model._trace is not None:  # parity tests read the features and, after backward(), their gradients
        sfeat.retain_grad()
        qfeat.retain_grad()
        model._trace.update(sfeat=sfeat, qfeat=qfeat)
    loss = ProtoHeadFn.apply(sfeat, qfeat, model, support_y, query_y)
    return model._train_logits, loss
