"""Training-mode forward of ProtoNet (reference models/protonet.py:245-275 under model.train()) and the autograd edge of its
head.  Compute lives in libr3d_hip.so (csrc/protonet_train.hip); this file orders launches: one episode under autograd
(protonet_train_forward), or the E episodes of an optimiser step as ONE launch sequence without the autograd engine
(explicit_train_batch, ProtoBatchTrainer).  Both run the same head, ProtoHeadFn: one episode is a batch of one."""
from types import SimpleNamespace

import torch

from . import ops, train_ops as T
from .ops import SegLayout


class ProtoHeadFn(torch.autograd.Function):
    """(sfeat, qfeat) -> cross-entropy loss (E,) of the prototype similarities, each the mean over ITS episode's query
    points; leaves logits / arg-max in model._train_logits / model._train_pred (E = 1: all without the episode axis).

    sfeat / qfeat: the support / query rows of episode 0; with ``ctx.E > 1`` (set by the caller) they are views into ONE
    feature matrix in which episode e's rows start ``ctx.ep_rows`` rows further on.  backward writes both feature
    gradients into ONE (E (S*N + n_q*N), D) matrix, per episode support rows then query rows -- the layout
    train_ops.EncoderTrainFn.backward consumes --, leaves it in ``ctx.dfeat_full`` and returns it whole (E > 1) or as its
    two row ranges."""

    @staticmethod
    def forward(ctx, sfeat, qfeat, model, support_y, query_y):
        E = getattr(ctx, "E", 1)
        ep_rows = getattr(ctx, "ep_rows", 0)
        N = model.n_points
        n_q = query_y.shape[-2]
        Z, ws = ops.protonet_head_train(sfeat, qfeat, support_y, model.n_way, model.k_shot, N, model.dist_method, n_ep=E,
                                        feat_ep_rows=ep_rows, n_query_pts=n_q * N)
        labels = query_y.reshape(E, n_q, N).to(torch.int64).contiguous()
        logits, loss, pred = ops.logits_ce_from_rows(Z, E, n_q, N, model.n_way + 1, labels)
        if E == 1:
            logits, loss, pred = logits[0], loss[0], pred[0]
        ctx.model, ctx.Z, ctx.ws, ctx.labels, ctx.n_q, ctx.E, ctx.ep_rows = model, Z, ws, labels, n_q, E, ep_rows
        ctx.qfeat, ctx.support_y = qfeat, support_y
        model._train_logits, model._train_pred = logits, pred
        return loss

    @staticmethod
    def backward(ctx, gloss):
        model, Z, n_q, E, ep_rows = ctx.model, ctx.Z, ctx.n_q, ctx.E, ctx.ep_rows
        dev = Z.device
        N, D = model.n_points, model.feat_dim
        S = model.n_way * model.k_shot
        zero = torch.zeros(1, device=dev, dtype=torch.int32)  # (no prototype rows in front of the query rows)
        G = ops.ce_grad(Z, zero, 0, E, n_q * N, n_q * N, model.n_way + 1, ctx.labels, gloss)
        assert E == 1 or ep_rows == (S + n_q) * N
        dfeat = torch.empty(E * (S + n_q) * N, D, device=dev, dtype=torch.float32)
        ops.protonet_head_bwd(ctx.qfeat, ctx.support_y, model.n_way, model.k_shot, N, model.dist_method, G, ctx.ws, dfeat,
                              dfeat[S * N:], n_ep=E, feat_ep_rows=ep_rows, dfeat_ep_rows=ep_rows, n_query_pts=n_q * N)
        ctx.dfeat_full = dfeat  # (explicit_train_batch takes the whole buffer)
        if E > 1:
            return dfeat, None, None, None, None
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


def explicit_train_batch(model, batch, grad_sink):
    """Forward + backward of the E episodes of `batch` (batch.EpisodeBatch) as ONE fixed launch sequence without the
    autograd engine (train_ops.explicit_encoder_step, as head_train.explicit_train_batch for MPTI): training encoder over
    all E (S + Q) clouds with BatchNorm batch statistics per episode and getFeatures call, the head kernels with n_ep = E,
    one cross entropy per episode (the mean over ITS query points) with a unit upstream gradient each, and every parameter
    gradient -- summed over the E episodes where it is produced -- ADDED into grad_sink[i].  Per episode the same kernels
    and results as protonet_train_forward + loss.backward(), episode after episode.
    Returns (loss (E,), logits (E, n_q, n_way + 1, N), pred (E, n_q, N) int32, correct (E,) int32)."""
    E, N = batch.E, model.n_points
    Q = batch.query_x.shape[1]

    def head(feat, seg):
        ctx = SimpleNamespace(E=E, ep_rows=seg.ep_rows)
        loss = ProtoHeadFn.forward(ctx, feat, feat[seg.rows_a:], model, batch.support_y, batch.query_y).reshape(E)
        logits, pred = model._train_logits.reshape(E, Q, model.n_way + 1, N), model._train_pred.reshape(E, Q, N)
        correct = ops.count_correct(pred, batch.query_y)
        ProtoHeadFn.backward(ctx, torch.ones((), device=feat.device))  # d(step loss) / d(loss_e) = 1 for every episode
        return (loss, logits, pred, correct), ctx.dfeat_full, []

    return T.explicit_encoder_step(model, batch, grad_sink, head)


class ProtoBatchTrainer:
    """What ProtoLearner.train_batch needs around explicit_train_batch: ONE flat gradient bucket (dist.FlatGradBucket: a
    single all-reduce carries the gradients and the episode count), the deferred BatchNorm running-statistics records and
    the optimiser step on the mean gradient.

    The parameters' .grad is bound to the bucket's views right before every optimiser step and not relied on in between:
    ProtoLearner.train() may have run since (its zero_grad() sets .grad to None and its backward() allocates fresh
    tensors), so a step here never reads another call's gradient and train() never writes into the bucket."""

    def __init__(self, learner, max_episodes=256):
        from . import dist as D
        self.learner, self.model = learner, learner.model
        self.bucket = D.FlatGradBucket(self.model.parameters())
        self.views = [p.grad for p in self.bucket.params]
        dev = self.bucket.store.device
        self.max_episodes = max_episodes
        self.bn_records = T.BNRecorder(max_episodes, dev)
        self.bn_records.index_dev = torch.zeros(1, device=dev, dtype=torch.int32)  # (one batch per step: records start at 0)

    def step(self, batch):
        """One optimiser step on the mean gradient of the batch's episodes (over all ranks' episodes when torch.distributed
        is initialised).  Returns explicit_train_batch's results."""
        from . import dist as D
        assert batch.E <= self.max_episodes
        self.model.train()
        self.bucket.zero_()
        saved, T.bn_recorder = T.bn_recorder, self.bn_records
        try:
            out = explicit_train_batch(self.model, batch, self.views)
        finally:
            T.bn_recorder = saved
        self.bucket.all_reduce_mean(batch.E)
        # the running statistics move only now that the step is known to be applied, in the order E single calls would
        # move them: episode after episode, support call then query call
        self.bn_records.apply(batch.E)
        D.mark_rank_local_stats(self.model)
        for p, v in zip(self.bucket.params, self.views):
            p.grad = v
        self.learner.optimizer.step()
        self.learner.lr_scheduler.step()
        return out
