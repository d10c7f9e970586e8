"""Training-mode forward of MPTI_SelfAtten (reference models/mpti.py:414-577 with train=True): the transductive head as
plain halves (lp_forward / lp_backward), their autograd adapter for one episode (HeadLPFn, behind mpti_train_forward) and
the explicit step that calls the halves of encoder, contrastive loss and head in order (explicit_train_batch).  Compute
lives in libr3d_hip.so; this file orders launches.

Like train_ops.py, everything here runs on a batch of E episodes (ops.SegLayout); E = 1 is the reference's schedule."""
from collections import namedtuple

import torch

from . import _lib, contrast, ops, train_ops as T
from .ops import SegLayout, _p, _st, _timed

LPSaved = namedtuple("LPSaved", "model hb labels n_q E ep_rows budget")


def lp_forward(model, sfeat, qfeat, support_y, query_y, E=1, ep_rows=0):
    """(sfeat, qfeat) -> (lp_loss (E,), logits (E, n_q, n_classes, N), pred (E, n_q, N) int32, saved); also leaves Z in the
    head buffers.  sfeat / qfeat: the support / query rows of episode 0; episode e's rows start e * ep_rows rows further
    on in the same matrix."""
    S, N = model.n_way * model.k_shot, model.n_points
    n_q = query_y.shape[-2]
    hb = model._head_buffers(n_q, sfeat.device, E)
    sy = support_y.reshape(E, S, N).to(torch.int32).contiguous()
    if model._lp_force:  # the conservative re-run (see MPTILearner_V3.train): one FPS launch per round as well
        hb.fps_one_launch = False
    ops.head_prototypes(hb, sy, None, sfeat, qfeat, ep_rows)
    # eval's graph and solve on eval's launch-budget policy (mpti.py: _propagate, _lp_next_budget); MPTILearner_V3.train /
    # DPTrainer.step check lp_converged(backward=True) before the optimiser step and redo the episode on this conservative
    # schedule
    budget = model._propagate(hb, exact=model._lp_force)
    labels = query_y.reshape(E, n_q, N).to(torch.int64).contiguous()
    logits, loss, pred = ops.query_logits_ce(hb, n_q, model.n_classes, labels)
    return loss, logits, pred, LPSaved(model, hb, labels, n_q, E, ep_rows, budget)


def lp_backward(saved, gscale):
    """d(gscale * sum_e lp_loss[e]) / d(features) as ONE matrix over the batch's rows, per episode support rows then query
    rows: the layout of the encoder's feat, which encoder_backward takes whole."""
    model, hb, labels, n_q, E, ep_rows, fwd_budget = saved
    lib = _lib.load()
    dev = hb.Z.device
    N, D = model.n_points, model.feat_dim
    S = model.n_way * model.k_shot
    pl = E * hb.n_cap  # rows of one plane of label columns (ops.HeadBuffers: two planes for more than 3 ways)
    G = ops.ce_grad(hb.Z, hb.n_proto_ptr(), ops.HD_WORDS, E, hb.n_cap, n_q * N, model.n_classes, labels, gscale)
    lam = torch.empty(pl, 4, device=dev, dtype=torch.float32)
    dnodes = torch.empty(pl, D, device=dev, dtype=torch.float32)
    budget = int(min(model.lp_max_iter, fwd_budget + max(4, fwd_budget // 4)))
    with _timed("label_propagate_bwd"):
        for plane in range(hb.planes):  # the adjoint is column-wise independent as well: the planes' dnodes add
            dn = dnodes if plane == 0 else torch.empty_like(dnodes)
            stats = hb.stats_bwd if plane == 0 else torch.zeros(E, 2, device=dev, dtype=torch.int32)
            _lib.check(lib.r3d_label_propagate_bwd_batched(
                E, _p(hb.nodes), hb.nodes.stride(0), D, hb.kp1, _p(hb.Z[plane * pl:]), _p(G[plane * pl:]),
                _p(hb.n_nodes_ptr()), ops.HD_WORDS, hb.n_cap, float(model.sigma), 0.99, budget, float(model.lp_tol), _p(lam), _p(dn),
                D, _p(hb.lp_ws), hb.lp_words, hb.lp_stride, _p(stats), 2, _st()))
            if plane:
                dnodes.add_(dn)
                hb.stats_bwd[:, 0] = torch.minimum(hb.stats_bwd[:, 0], stats[:, 0])
                hb.stats_bwd[:, 1] = torch.maximum(hb.stats_bwd[:, 1], stats[:, 1])
    assert E == 1 or ep_rows == (S + n_q) * N
    rows = E * (S + n_q) * N
    dfeat = torch.empty(rows, D, device=dev, dtype=torch.float32)
    dfeat.view(E, (S + n_q) * N, D)[:, :S * N].zero_()
    dsfeat, dqfeat = dfeat, dfeat[S * N:]
    _lib.check(lib.r3d_head_prototypes_bwd_batched(E, _p(dnodes), D, hb.n_cap, model.n_way, model.k_shot, N, D, n_q * N,
                                                   _p(hb.desc), ops.HD_WORDS, _p(hb.assign), 2 * S * N, _p(hb.cluster_count), hb.n_cap,
                                                   _p(hb.proto_ws), hb.proto_stride, _p(dsfeat), D, ep_rows, _p(dqfeat), D,
                                                   ep_rows, _st()))
    return dfeat


class HeadLPFn(torch.autograd.Function):
    """The autograd adapter of lp_forward / lp_backward for ONE episode: (sfeat, qfeat) -> lp_loss (0-d).  The logits and
    their arg-max, which carry no gradient, wait in ``model._train_out`` for mpti_train_forward."""

    @staticmethod
    def forward(ctx, sfeat, qfeat, model, support_y, query_y):
        loss, logits, pred, ctx.saved = lp_forward(model, sfeat, qfeat, support_y, query_y)
        model._train_out, ctx.rows = (logits[0], pred[0]), sfeat.shape[0]
        return loss[0]

    @staticmethod
    def backward(ctx, gloss):
        dfeat = lp_backward(ctx.saved, gloss)
        return dfeat[:ctx.rows], dfeat[ctx.rows:], None, None, None


def mpti_train_forward(model, support_x, support_y, query_x, query_y, gt_support_y, gt_query_y, logger, support_flag):
    """Returns the reference's 7-tuple (mpti.py:573-575): query_pred, lp_loss, contrast_loss, query_acc_LP,
    query_acc_original, clean_ratio_LP_avg, clean_ratio_original_avg."""
    S, N = model.n_way * model.k_shot, model.n_points
    seed = T.next_dropout_seed(model)  # (captured launch sequence: the seed advances in device memory)
    sx = support_x.reshape(S, model.in_channels, N)
    # two getFeatures calls, each with its own BatchNorm batch statistics (mpti.py:434,436), through one launch sequence
    # over the S + Q clouds
    seg = SegLayout(1, S, query_x.shape[0], N)
    sfeat, qfeat = T.get_features_train(model, ops.cat_clouds(sx, query_x, 0), seed, seg=seg)
    if model._trace is not None:  # parity tests read the features and, after backward(), their gradients
        sfeat.retain_grad()
        qfeat.retain_grad()
        model._trace.update(sfeat=sfeat, qfeat=qfeat)
    contrast_loss = contrast.per_way_contrast_loss(model, sfeat, support_y, support_flag)
    lp_loss = HeadLPFn.apply(sfeat, qfeat, model, support_y, query_y)
    logits, pred = model._train_out
    metrics = contrast.train_debug_metrics(model, model._head[1], pred, support_y, gt_support_y, query_y, gt_query_y, logger)
    return (logits, lp_loss, contrast_loss) + tuple(metrics[0].unbind(0))


def explicit_train_batch(model, batch, grad_sink, loss_weight=0.1):
    """Forward + backward of the E episodes of `batch` (batch.EpisodeBatch) as ONE fixed launch sequence without the
    autograd engine (train_ops.explicit_encoder_step): the forward halves of encoder, contrastive loss and head, then
    their backward halves in dependency order, and every parameter gradient -- summed over the E episodes where it is
    produced -- is ADDED into grad_sink[i] (views in the order of model.parameters(), requires_grad only).  Same
    kernels and, per episode, the same results as ``loss = lp + loss_weight * contrast; loss.backward()``
    (models/mpti_learner.py:66-68) episode after episode.  Returns (loss (E,), logits (E, n_q, n_classes, N),
    metrics (E, 4), lp_loss (E,), contrast_loss (E,))."""
    E = batch.E

    def head(feat, seg):
        sfeat, qfeat = feat, feat[seg.rows_a:]
        closs, csaved = contrast.contrast_forward(model, sfeat, model.proj.weight, model.proj.bias, batch.support_y,
                                                  batch.support_flag, E, seg.ep_rows)
        lploss, logits, pred, lsaved = lp_forward(model, sfeat, qfeat, batch.support_y, batch.query_y, E, seg.ep_rows)
        metrics = contrast.train_debug_metrics(model, lsaved.hb, pred, batch.support_y, batch.gt_support_y, batch.query_y,
                                               batch.gt_query_y)
        loss = lploss + loss_weight * closs
        # ---- backward, in dependency order
        one = torch.ones((), device=feat.device)
        # (the contrast gradient over all rows of the batch, zero on the query rows: the layout of `feat` too)
        dfeat_c, dWp, dbp = contrast.contrast_backward(csaved, one * loss_weight, feat.shape[0])
        dfeat = lp_backward(lsaved, one)
        dfeat.add_(dfeat_c)
        return (loss, logits, metrics, lploss, closs), dfeat, [(model.proj.weight, dWp), (model.proj.bias, dbp)]

    return T.explicit_encoder_step(model, batch, grad_sink, head)


def explicit_train_episode(model, episode, grad_sink, loss_weight=0.1):
    """One episode (train layout, loader.py:1666-1671) through explicit_train_batch: the launch sequence that
    episode_graph.EpisodeGraphs freezes into a hipGraph.  Returns (loss, logits, metrics[4], lp_loss, contrast_loss)."""
    from .batch import EpisodeBatch
    model._lp_force = False  # a frozen launch sequence always runs on the slot's fixed budget
    b = EpisodeBatch.from_episodes([episode])
    loss, logits, metrics, lp, con = explicit_train_batch(model, b, grad_sink, loss_weight)
    return loss.reshape(()), logits[0], tuple(metrics.reshape(4).unbind(0)), lp.reshape(()), con.reshape(())
