"""Host-side mirror of the reference's models/protonet.py::ProtoNet (lines 39-58, 245-354):
same constructor and forward() signature; encoder / attention / base learner run on the HIP
kernels (dgcnn.FewShotFeatures), the head is r3d_protonet_head_batched (evaluation: _forward_eval, a single episode is a
batch of one) or r3d_protonet_head_train_fwd / r3d_protonet_head_bwd (a module in .train() mode: protonet_train.py).

ProtoNet_Contrast (models/protonet.py:357-946, "protonet+CCNS+MDNS") is the same evaluation with the clean-shot detection
in front of the head: r3d_clean_shot_detect_batched, then r3d_protonet_head_keep_batched.  Evaluation only."""
import torch
from torch import nn

from . import ops
from .dgcnn import FewShotFeatures


class ProtoNet(FewShotFeatures):
    detect_clean_shots = False  # ProtoNet_Contrast: the clean-shot detection decides which shots form a way's prototype
    fit_table = "protos"        # the field of a fitted.FittedSupport this model's predict reads

    def __init__(self, args):
        super().__init__(args)
        self.dist_method = args.dist_method

    def forward(self, support_x, support_y, query_x, query_y, support_c=None, query_c=None, train=False,
                gt_support_y=None, gt_query_y=None, logger=None):
        if train and not self.training:
            raise NotImplementedError("train=True needs model.train(): the training kernels use batch-statistics "
                                      "BatchNorm and attention dropout (models/mpti_learner.py:58-63)")
        if self.training:  # the reference's forward under model.train(): the same pair, the loss carries the graph
            if not self.use_attention:
                raise NotImplementedError("training with use_attention=False (the linear mapper) is not built: the training "
                                          "encoder (train_ops.encoder_forward) needs the attention learner")
            from . import protonet_train
            return protonet_train.protonet_train_forward(self, support_x, support_y, query_x, query_y)
        logits, loss, _ = self._forward_eval(support_x[None], support_y[None], query_x[None],
                                             query_y[None] if query_y is not None else None)
        return logits[0], loss[0]

    def forward_episodes(self, batch):
        """Inference forward of the E episodes of `batch` (batch.EpisodeBatch) in ONE launch sequence.  Returns (logits
        (E, n_q, n_way + 1, N), loss (E,), pred (E, n_q, N) int32, correct (E,) int32): per episode what forward() gives
        for it."""
        if self.training:
            raise NotImplementedError("forward_episodes is the inference path; training batches go through "
                                      "protonet_train.explicit_train_batch")
        logits, loss, pred = self._forward_eval(batch.support_x, batch.support_y, batch.query_x, batch.query_y)
        return logits, loss, pred, ops.count_correct(pred, batch.query_y)

    def _forward_eval(self, support_x, support_y, query_x, query_y):
        """support_x (E, n_way, k_shot, C, N), support_y (E, n_way, k_shot, N), query_x (E, n_q, C, N), query_y (E, n_q, N) or
        None -> logits (E, n_q, n_way + 1, N), loss (E,), pred (E, n_q, N) int32."""
        E = support_x.shape[0]
        S, N = self.n_way * self.k_shot, self.n_points
        n_q = query_x.shape[1]
        sx = support_x.reshape(E, S, self.in_channels, N)
        # eval-mode BatchNorm uses running statistics, so all clouds of all episodes share one encoder pass; rows per
        # episode: its S support clouds, then its n_q query clouds
        feat = self.getFeatures_pm(ops.cat_clouds(sx, query_x, 1).reshape(E * (S + n_q), self.in_channels, N), group=S + n_q)
        shot_keep = None
        if self.detect_clean_shots:  # Mean_pl_support_y_multi_scale (protonet.py:491-565): the decision rule of mpti.py:178-223
            shot_keep = ops.clean_shot_detect(feat, sx, support_y, self.n_way, self.k_shot, N, E=E, feat_ep_rows=(S + n_q) * N)
        if self._trace is not None:
            self._trace.update(feat=feat, shot_keep=shot_keep)
        Z = ops.protonet_head_batched(feat, feat[S * N:], support_y, self.n_way, self.k_shot, N, self.dist_method, E,
                                      (S + n_q) * N, n_q * N, shot_keep=shot_keep)
        labels = query_y.reshape(E, n_q, N).to(torch.int64).contiguous() if query_y is not None else None
        return ops.logits_ce_from_rows(Z, E, n_q, N, self.n_way + 1, labels)

    # ------------------------------------------------------------------ a support set fitted once (fitted.py)
    def fit_support(self, support_x, support_y, eval=False, lp_iters=None, n_queries=None):
        """The support half of _forward_eval, once: encoder over the S support clouds, clean-shot detection
        (ProtoNet_Contrast: always; ProtoNet: never -- `eval` and `lp_iters` are MPTI's and ignored here), masked pooling and
        prototypes -> fitted.FittedSupport owning the (1, n_way + 1, D) table.  n_queries: the query clouds per group predict
        will be called with, if known (default n_way, the reference's episodes): the attention then splits its key axis as
        forward() does on the full episode (attention.hip: moot under the default of no split)."""
        from . import fitted as F
        S, N = F.check_fit_args(self, support_x, support_y), self.n_points
        sx = support_x.reshape(S, self.in_channels, N)
        feat = self.getFeatures_pm(sx, group=S + (n_queries or self.n_way))
        shot_keep = None
        if self.detect_clean_shots:
            shot_keep = ops.clean_shot_detect(feat, sx, support_y, self.n_way, self.k_shot, N)
        protos = ops.protonet_prototypes(feat, support_y, self.n_way, self.k_shot, N, shot_keep=shot_keep)
        return F.FittedSupport(self, protos=protos, shot_keep=shot_keep, eval=eval, n_queries=n_queries)

    def _predict_groups(self, fitted, query_x, query_y, lp_iters=None):
        """query_x (G, n_q, C, N), query_y (G, n_q, N) or None -> logits (G, n_q, n_way + 1, N), loss (G,), pred (G, n_q, N)
        int32: G groups against ONE fitted table in one launch sequence (encoder over the G n_q query clouds, similarity)."""
        G, n_q, N = query_x.shape[0], query_x.shape[1], self.n_points
        feat = self._query_features(query_x)
        Z = ops.protonet_similarity(feat, fitted.protos, self.n_way, self.dist_method, G, n_q * N)
        labels = query_y.reshape(G, n_q, N).to(torch.int64).contiguous() if query_y is not None else None
        return ops.logits_ce_from_rows(Z, G, n_q, N, self.n_way + 1, labels)

    def _predict_groups_sets(self, fits, query_x, lp_iters=None):
        """_predict_groups against K fitted tables with ONE encoder pass: fits: fitted.FittedSets (or a list of
        FittedSupports), query_x (G, n_q, C, N) -> logits (G, K, n_q, n_way + 1, N); [:, k] has the bits of
        _predict_groups(fits[k], query_x).  One similarity launch scores every query row against all K tables."""
        from . import fitted as F
        fits = fits if isinstance(fits, F.FittedSets) else F.FittedSets(fits)
        if fits.table is None:
            fits.table = torch.cat([f.protos.reshape(1, self.n_way + 1, -1) for f in fits]).contiguous()
        G, n_q, N, K = query_x.shape[0], query_x.shape[1], self.n_points, len(fits)
        feat = self._query_features(query_x)
        Z = ops.protonet_similarity_sets(feat, fits.table, self.n_way, self.dist_method, G, n_q * N)
        return ops.logits_ce_from_rows(Z, G * K, n_q, N, self.n_way + 1, None)[0].reshape(G, K, n_q, self.n_way + 1, N)

    def predict(self, fitted, query_x, query_y=None, lp_iters=None):
        """Segment query clouds against a fitted support set: query_x (n_q, C, N) -> (logits (n_q, n_way + 1, N), loss), or
        (G, n_q, C, N) -> (logits (G, n_q, n_way + 1, N), loss (G,)); any n_q >= 1; loss is None without query_y.  Per group
        the bits of forward() on the episode [that support set | that group].  ValueError, before any launch, for a shape
        that does not match the fit or a fit whose weights have changed since (fitted.py)."""
        from . import fitted as F
        _, _, grouped = F.check_predict_args(self, fitted, query_x, query_y)
        if fitted.protos is None:
            raise ValueError("predict: the fit holds no prototype table (it was fitted by %s)" % fitted.model_class)
        qx = query_x if grouped else query_x[None]
        qy = query_y if (grouped or query_y is None) else query_y[None]
        logits, loss, _ = self._predict_groups(fitted, qx, qy, lp_iters)
        if not grouped:
            logits, loss = logits[0], loss[0]
        return logits, (loss if query_y is not None else None)


class ProtoNet_Contrast(ProtoNet):
    """The reference's noise-robust baseline at test time: ProtoNet whose foreground prototypes average the shots the
    clean-shot detection kept (getPrototype(clean_flag=...), protonet.py:892-915); the background prototype takes every
    shot.  State-dict names are the reference's, `proj` (the contrastive projection, used in training only) included, so a
    checkpoint saved from the reference class loads strictly.  Training (`train=True`: per_way_contrast_loss) is not built:
    the reference has no learner that runs it."""
    detect_clean_shots = True

    def __init__(self, args):
        super().__init__(args)
        # the reference hard-codes feat_dim = 192 (protonet.py:382) for proj and for the clean_flag mask of getPrototype
        if self.feat_dim != 192:
            raise NotImplementedError("ProtoNet_Contrast: the reference fixes feat_dim = 192 (proj is Linear(192, 128), "
                                      "models/protonet.py:382-383); these widths give %d, which no checkpoint of it matches"
                                      % self.feat_dim)
        self.proj = nn.Linear(self.feat_dim, 128)

    def forward(self, support_x, support_y, query_x, query_y, gt_support_y=None, gt_query_y=None, train=False, logger=None,
                step=None, path=None, sampled_classes=None, bg_pcd_x=None, bg_pcd_y=None, support_c=None, support_flag=None,
                pcd_1024=None, label_1024=None, pcd_cutout=None, label_cutout=None):
        if train or self.training:
            raise NotImplementedError("ProtoNet_Contrast is built for evaluation (train=False on a module in .eval() mode): "
                                      "its train=True branch (per_way_contrast_loss) needs a learner the reference does not "
                                      "have; train the checkpoint as ProtoNet")
        logits, loss, _ = self._forward_eval(support_x[None], support_y[None], query_x[None],
                                             query_y[None] if query_y is not None else None)
        return logits[0], loss[0]
