"""Training-mode forward of ProtoNet (reference models/protonet.py:245-275 under model.train()) and the autograd edge of its
head.  Compute lives in libr3d_hip.so (csrc/protonet_train.hip); this file orders launches: one episode under autograd
(protonet_train_forward), or the E episodes of an optimiser step as ONE launch sequence without the autograd engine
(explicit_train_batch, ProtoBatchTrainer)."""
from types import SimpleNamespace

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


def explicit_train_batch(model, batch, grad_sink):
    """Forward + backward of the E episodes of `batch` (batch.EpisodeBatch) as ONE fixed launch sequence without the
    autograd engine (as head_train.explicit_train_batch for MPTI): training encoder over all E (S + Q) clouds with BatchNorm
    batch statistics per episode and getFeatures call, the head kernels with n_ep = E, one cross entropy per episode (the
    mean over ITS query points) with a unit upstream gradient each, and every parameter gradient -- summed over the E
    episodes where it is produced -- ADDED into grad_sink[i] (views in the order of model.parameters(), requires_grad
    only).  Per episode the same kernels and results as protonet_train_forward + loss.backward(), episode after episode.
    Returns (loss (E,), logits (E, n_q, n_way + 1, N), pred (E, n_q, N) int32, correct (E,) int32)."""
    E = batch.E
    S, N, D = model.n_way * model.k_shot, model.n_points, model.feat_dim
    Q = batch.query_x.shape[1]
    n_pts, C = Q * N, model.n_way + 1
    with torch.no_grad():
        seed = T.next_dropout_seeds(model, E)
        params = T.encoder_params(model)
        ctx = SimpleNamespace(param_list=params)
        seg = ctx.seg = SegLayout(E, S, Q, N)
        feat = T.EncoderTrainFn.forward(ctx, batch.x_all.view(E * (S + Q), model.in_channels, N), model, seed)
        sfeat, qfeat = feat, feat[S * N:]
        Z, ws = ops.protonet_head_train(sfeat, qfeat, batch.support_y, model.n_way, model.k_shot, N, model.dist_method, n_ep=E,
                                        feat_ep_rows=seg.ep_rows, n_query_pts=n_pts)
        logits, loss, pred = ops.logits_ce_from_rows_batched(Z, E, Q, N, C, batch.query_y)
        correct = ops.count_correct(pred, batch.query_y)
        # ---- backward, in dependency order
        dev = feat.device
        one = torch.ones(1, device=dev, dtype=torch.float32)  # d(step loss) / d(loss_e) = 1 for every episode
        zero = torch.zeros(1, device=dev, dtype=torch.int32)  # (no prototype rows in front of the query rows)
        G = torch.empty_like(Z)
        _lib.check(_lib.load().r3d_ce_grad_batched(E, _p(Z), _p(zero), 0, n_pts, n_pts, C, _p(batch.query_y), _p(one), _p(G), _st()))
        dfeat = torch.empty(E * seg.ep_rows, D, device=dev, dtype=torch.float32)  # the layout of `feat`
        ops.protonet_head_bwd(qfeat, batch.support_y, model.n_way, model.k_shot, N, model.dist_method, G, ws, dfeat, dfeat[S * N:],
                              n_ep=E, feat_ep_rows=seg.ep_rows, dfeat_ep_rows=seg.ep_rows, n_query_pts=n_pts)
        grads = T.EncoderTrainFn.backward(ctx, dfeat)[3:]
        index = {id(p): i for i, p in enumerate(q for q in model.parameters() if q.requires_grad)}
        dst, src = [], []
        for p, g in zip(params, grads):
            if g is not None:
                dst.append(grad_sink[index[id(p)]])
                src.append(g.reshape(p.shape))
        torch._foreach_add_(dst, src)
    return loss, logits, pred, correct


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
