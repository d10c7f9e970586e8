"""Training-mode forward of ProtoNet (reference models/protonet.py:245-275 under model.train()): its head as plain halves
(proto_forward / proto_backward; compute in libr3d_hip.so, csrc/protonet_train.hip) and the two callers that order the
launches: one episode under autograd (protonet_train_forward, through the adapter ProtoHeadFn), or the E episodes of an
optimiser step as ONE launch sequence without the autograd engine (explicit_train_batch, ProtoBatchTrainer).  Both run
the same halves: one episode is a batch of one."""
from collections import namedtuple

import torch

from . import ops, train_ops as T
from .ops import SegLayout

ProtoSaved = namedtuple("ProtoSaved", "model Z ws labels n_q E ep_rows qfeat support_y")


def proto_forward(model, sfeat, qfeat, support_y, query_y, E=1, ep_rows=0):
    """(sfeat, qfeat) -> (loss (E,), logits (E, n_q, n_way + 1, N), pred (E, n_q, N) int32, saved): the cross entropy of the
    prototype similarities, each the mean over ITS episode's query points, and their arg-max.  sfeat / qfeat: the support /
    query rows of episode 0; episode e's rows start e * ep_rows rows further on in the same matrix."""
    N = model.n_points
    n_q = query_y.shape[-2]
    Z, ws = ops.protonet_head_train(sfeat, qfeat, support_y, model.n_way, model.k_shot, N, model.dist_method, n_ep=E,
                                    feat_ep_rows=ep_rows, n_query_pts=n_q * N)
    labels = query_y.reshape(E, n_q, N).to(torch.int64).contiguous()
    logits, loss, pred = ops.logits_ce_from_rows(Z, E, n_q, N, model.n_way + 1, labels)
    return loss, logits, pred, ProtoSaved(model, Z, ws, labels, n_q, E, ep_rows, qfeat, support_y)


def proto_backward(saved, gscale):
    """d(gscale * sum_e loss[e]) / d(features) as ONE (E (S*N + n_q*N), D) matrix, per episode support rows then query
    rows -- the layout train_ops.encoder_backward consumes."""
    model, Z, ws, labels, n_q, E, ep_rows, qfeat, support_y = saved
    dev = Z.device
    N, D = model.n_points, model.feat_dim
    S = model.n_way * model.k_shot
    zero = torch.zeros(1, device=dev, dtype=torch.int32)  # (no prototype rows in front of the query rows)
    G = ops.ce_grad(Z, zero, 0, E, n_q * N, n_q * N, model.n_way + 1, labels, gscale)
    assert E == 1 or ep_rows == (S + n_q) * N
    dfeat = torch.empty(E * (S + n_q) * N, D, device=dev, dtype=torch.float32)
    ops.protonet_head_bwd(qfeat, support_y, model.n_way, model.k_shot, N, model.dist_method, G, ws, dfeat, dfeat[S * N:],
                          n_ep=E, feat_ep_rows=ep_rows, dfeat_ep_rows=ep_rows, n_query_pts=n_q * N)
    return dfeat


class ProtoHeadFn(torch.autograd.Function):
    """The autograd adapter of proto_forward / proto_backward for ONE episode: (sfeat, qfeat) -> loss (0-d).  The logits,
    which carry no gradient, wait in ``model._train_out`` for protonet_train_forward."""

    @staticmethod
    def forward(ctx, sfeat, qfeat, model, support_y, query_y):
        loss, logits, pred, ctx.saved = proto_forward(model, sfeat, qfeat, support_y, query_y)
        model._train_out, ctx.rows = (logits[0], pred[0]), sfeat.shape[0]
        return loss[0]

    @staticmethod
    def backward(ctx, gloss):
        dfeat = proto_backward(ctx.saved, gloss)
        return dfeat[:ctx.rows], dfeat[ctx.rows:], None, None, None


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
    return model._train_out[0], loss


def explicit_train_batch(model, batch, grad_sink):
    """Forward + backward of the E episodes of `batch` (batch.EpisodeBatch) as ONE fixed launch sequence without the
    autograd engine (train_ops.explicit_encoder_step, as head_train.explicit_train_batch for MPTI): training encoder over
    all E (S + Q) clouds with BatchNorm batch statistics per episode and getFeatures call, the head kernels with n_ep = E,
    one cross entropy per episode (the mean over ITS query points) with a unit upstream gradient each, and every parameter
    gradient -- summed over the E episodes where it is produced -- ADDED into grad_sink[i].  Per episode the same kernels
    and results as protonet_train_forward + loss.backward(), episode after episode.
    Returns (loss (E,), logits (E, n_q, n_way + 1, N), pred (E, n_q, N) int32, correct (E,) int32)."""
    def head(feat, seg):
        loss, logits, pred, saved = proto_forward(model, feat, feat[seg.rows_a:], batch.support_y, batch.query_y, batch.E,
                                                  seg.ep_rows)
        correct = ops.count_correct(pred, batch.query_y)
        dfeat = proto_backward(saved, torch.ones((), device=feat.device))  # d(step loss) / d(loss_e) = 1 for every episode
        return (loss, logits, pred, correct), dfeat, []

    return T.explicit_encoder_step(model, batch, grad_sink, head)


class ProtoBatchTrainer:
    """What ProtoLearner.train_batch needs around explicit_train_batch: ONE flat gradient bucket (dist.FlatGradBucket),
    ProtoNet's deferred BatchNorm running-statistics records, and the tail every optimiser step shares
    (dp_train.reduce_and_step: one all-reduce carries the gradients and the episode count; .grad is bound to the bucket's
    views right before the optimiser step and not relied on in between, so ProtoLearner.train() may run in between)."""

    def __init__(self, learner, max_episodes=256):
        from . import dist as D
        self.learner, self.model = learner, learner.model
        self.bucket = D.FlatGradBucket(self.model.parameters())
        dev = self.bucket.store.device
        self.max_episodes = max_episodes
        self.bn_records = T.BNRecorder(max_episodes, dev)
        self.bn_records.index_dev = torch.zeros(1, device=dev, dtype=torch.int32)  # (one batch per step: records start at 0)

    def step(self, batch):
        """One optimiser step on the mean gradient of the batch's episodes (over all ranks' episodes when torch.distributed
        is initialised).  Returns explicit_train_batch's results."""
        from .dp_train import reduce_and_step
        assert batch.E <= self.max_episodes
        self.model.train()
        self.bucket.zero_()
        with T.recording(self.bn_records):
            out = explicit_train_batch(self.model, batch, self.bucket.views)
        # (the records apply as E single calls would move the statistics: episode after episode, support then query call)
        reduce_and_step(self.learner, self.bucket, batch.E, apply_stats=lambda: self.bn_records.apply(batch.E))
        return out
