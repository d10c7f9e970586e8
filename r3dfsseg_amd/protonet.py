"""Host-side mirror of the reference's models/protonet.py::ProtoNet (lines 39-58, 245-354):
same constructor and forward() signature; encoder / attention / base learner run on the HIP
kernels, the head is r3d_protonet_head (evaluation; r3d_protonet_head_batched for a batch of episodes: forward_episodes)
or r3d_protonet_head_train_fwd / r3d_protonet_head_bwd (a module in .train() mode: protonet_train.py)."""
import torch
import torch.nn as nn

from . import ops
from .dgcnn import DGCNN, BaseLearner, SelfAttention, check_output_dim
from .mpti import EpisodeSlot


class ProtoNet(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.n_way = args.n_way
        self.k_shot = args.k_shot
        self.dist_method = args.dist_method
        self.in_channels = args.pc_in_dim
        self.n_points = args.pc_npts
        self.use_attention = args.use_attention
        if self.n_way > 7:
            raise NotImplementedError("n_way <= 7 (the head kernels carry at most 8 classes)")
        self.output_dim = args.output_dim
        self.feat_dim = args.edgeconv_widths[0][-1] + args.output_dim + args.base_widths[-1]
        check_output_dim(self.output_dim, self.use_attention, self.feat_dim)
        self.encoder = DGCNN(args.edgeconv_widths, args.dgcnn_mlp_widths, args.pc_in_dim, k=args.dgcnn_k)
        self.base_learner = BaseLearner(args.dgcnn_mlp_widths[-1], args.base_widths)
        if self.use_attention:
            self.att_learner = SelfAttention(args.dgcnn_mlp_widths[-1], args.output_dim)
        else:
            self.linear_mapper = nn.Conv1d(args.dgcnn_mlp_widths[-1], args.output_dim, 1, bias=False)
        self._slot = EpisodeSlot(0)  # what train_ops.EncoderTrainFn reads: the device word behind the dropout seed
        # parity tests set this to a dict; a training forward then leaves its neighbour lists and features in it
        self._trace = None

    def getFeatures_pm(self, x, group=0):
        """group > 0: x is a batch of episodes of `group` clouds each (the attention then splits its key axis as for one
        episode)."""
        B, _, N = x.shape
        x_pm, x_cm = ops.input_layouts(x)
        cat, level2 = self.encoder.forward_pm(x_pm, B, N, x_cm=x_cm)
        feat = torch.empty(B * N, self.feat_dim, device=x.device, dtype=torch.float32)
        d1, od = 64, self.output_dim
        ops.copy_cols(cat[:, :d1], feat[:, :d1])
        if self.use_attention:
            self.att_learner.forward_pm(level2, B, N, feat[:, d1:d1 + od], group=group)
        else:
            W = self.linear_mapper.weight.reshape(od, -1).contiguous()
            ops.pointwise_conv(level2, W, None, None, ops.ACT_NONE, out=feat[:, d1:d1 + od])
        self.base_learner.forward_pm(level2, feat[:, d1 + od:])
        return feat

    def getFeatures(self, x):
        B, _, N = x.shape
        return ops.pm_to_cm(self.getFeatures_pm(x), B, N)

    def forward(self, support_x, support_y, query_x, query_y, support_c=None, query_c=None, train=False,
                gt_support_y=None, gt_query_y=None, logger=None):
        if train and not self.training:
            raise NotImplementedError("train=True needs model.train(): the training kernels use batch-statistics "
                                      "BatchNorm and attention dropout (models/mpti_learner.py:58-63)")
        if self.training:  # the reference's forward under model.train(): the same pair, the loss carries the graph
            if not self.use_attention:
                raise NotImplementedError("training with use_attention=False (the linear mapper) is not built: the training "
                                          "encoder (train_ops.EncoderTrainFn) needs the attention learner")
            from . import protonet_train
            return protonet_train.protonet_train_forward(self, support_x, support_y, query_x, query_y)
        S, N = self.n_way * self.k_shot, self.n_points
        n_q = query_x.shape[0]
        sx = support_x.reshape(S, self.in_channels, N)
        feat = self.getFeatures_pm(torch.cat((sx, query_x), 0))
        Z = ops.protonet_head(feat[:S * N], feat[S * N:], support_y, self.n_way, self.k_shot, N, self.dist_method)
        labels = query_y.to(torch.int64).contiguous() if query_y is not None else None
        logits, loss, _ = ops.logits_ce_from_rows(Z, n_q, N, self.n_way + 1, labels)
        return logits, loss

    def forward_episodes(self, batch):
        """Inference forward of the E episodes of `batch` (batch.EpisodeBatch) in ONE launch sequence: eval-mode BatchNorm
        uses running statistics, so all clouds of all episodes share one encoder pass; then the batched head and the
        batched loss kernel.  Returns (logits (E, n_q, n_way + 1, N), loss (E,), pred (E, n_q, N) int32, correct (E,) int32):
        per episode what forward() gives for it."""
        if self.training:
            raise NotImplementedError("forward_episodes is the inference path; training batches go through "
                                      "protonet_train.explicit_train_batch")
        E = batch.E
        S, N = self.n_way * self.k_shot, self.n_points
        n_q = batch.query_x.shape[1]
        feat = self.getFeatures_pm(batch.x_all.reshape(E * (S + n_q), self.in_channels, N), group=S + n_q)
        Z = ops.protonet_head_batched(feat, feat[S * N:], batch.support_y, self.n_way, self.k_shot, N, self.dist_method, E,
                                      (S + n_q) * N, n_q * N)
        logits, loss, pred = ops.logits_ce_from_rows_batched(Z, E, n_q, N, self.n_way + 1, batch.query_y)
        return logits, loss, pred, ops.count_correct(pred, batch.query_y)
