"""Host-side mirror of the reference's models/proto_learner.py::ProtoLearner: test(), and the training loop train()
plainly intends (forward, zero_grad, backward, optimizer.step, lr_scheduler.step).  train_batch() / test_batch() are this
build's additions: E episodes of one shape per call through ONE launch sequence (protonet_train.explicit_train_batch,
ProtoNet.forward_episodes), as MPTILearner_V3.train_batch / test_batch."""
import torch
from torch import optim

from .checkpoint_util import load_model_checkpoint, load_pretrain_checkpoint
from .fitted import FittedLearner
from .metrics import point_accuracy
from .protonet import ProtoNet


class ProtoEvalBatch(FittedLearner):
    """The evaluation half ProtoLearner and ProtoContrastLearner share: E episodes of one shape through
    self.model.forward_episodes, and fit() / predict() (fitted.FittedLearner: a support set fitted once).  Needs self.model
    only."""

    @staticmethod
    def _batch(datas):
        """A list of episodes (the first four tensors of each are used) -> batch.EpisodeBatch on the device."""
        from .batch import EpisodeBatch
        if isinstance(datas, EpisodeBatch):
            return datas
        if len(datas) == 0:
            raise ValueError("an empty list of episodes: a batch is at least one episode")
        eps = [[t.cuda() for t in d[:4]] for d in datas]
        for e, ep in enumerate(eps[1:], 1):
            for i, (a, b) in enumerate(zip(eps[0], ep)):
                if a.shape != b.shape:
                    raise ValueError("a batch is E episodes of ONE shape: tensor %d of episode %d is %s, of episode 0 %s"
                                     % (i, e, tuple(b.shape), tuple(a.shape)))
        return EpisodeBatch.from_episodes(eps)

    def test_batch(self, datas, sampled_classes=None):
        """test() for E episodes of one shape in ONE launch sequence (ProtoNet.forward_episodes): a list of
        (pred (n_q, N), loss, accuracy), per episode what test() returns for it."""
        from . import dist as D
        b = self._batch(datas)
        self.model.eval()
        D.warn_rank_local_stats(self.model, 'evaluation')
        with torch.no_grad():
            _, loss, pred, correct = self.model.forward_episodes(b)
            pred = pred.to(torch.int64)
        n = b.query_y.shape[1] * b.query_y.shape[2]
        return [(pred[e], loss[e], c / n) for e, c in enumerate(correct.tolist())]  # (the batch's one host read)


class ProtoLearner(ProtoEvalBatch):
    def __init__(self, args, mode='train'):
        self.model = ProtoNet(args)
        self._batch_trainer = None  # protonet_train.ProtoBatchTrainer behind train_batch
        from .augment import LearnerAugment
        self._augm = LearnerAugment(args)  # args.device_augm (+ args.pc_augm): --pc_augm on the device, train*() only
        if not torch.cuda.is_available():
            raise RuntimeError("ProtoLearner needs an MI355X: the forward pass has no CPU path")
        self.model.cuda()
        synthetic = 'synthetic' in (getattr(args, 'pretrain_checkpoint_path', None), getattr(args, 'model_checkpoint_path', None))
        if synthetic:
            from . import synthetic as S
            sd = S.make_state_dict(vars(args))
            self.model.load_state_dict({k: v for k, v in sd.items() if not k.startswith('proj.')})
        if mode == 'train':
            head = self.model.att_learner if args.use_attention else self.model.linear_mapper
            self.optimizer = torch.optim.Adam(
                [{'params': self.model.encoder.parameters(), 'lr': 0.0001},
                 {'params': self.model.base_learner.parameters()},
                 {'params': head.parameters()}], lr=args.lr)
            self.lr_scheduler = optim.lr_scheduler.StepLR(self.optimizer, step_size=args.step_size, gamma=args.gamma)
            if not synthetic:
                self.model = load_pretrain_checkpoint(self.model, args.pretrain_checkpoint_path)
        elif mode == 'test':
            if not synthetic:
                self.model = load_model_checkpoint(self.model, args.model_checkpoint_path, mode='test')
        else:
            raise ValueError('Wrong GMMLearner mode (%s)! Option:train/test' % mode)

    def train(self, data, logger):
        """One optimisation step on one episode (models/proto_learner.py:55-67): model.train(), forward, zero_grad,
        loss.backward(), optimizer.step(), lr_scheduler.step().  Returns ``(loss, accuracy)``: the loss of the forward on the
        pre-step weights and the arg-max accuracy of that forward over all query points, background included.  These are the
        two values ProtoNet.forward can supply; the four further names in the reference's return statement
        (proto_learner.py:69: clean_ratio, size_ratio, query_acc_LP, query_acc_original) have no source in it.

        data: the 8-entry list of proto_learner.py:54 or the 11-tensor training layout (synthetic.make_episode(train=True),
        the reference's training collate); only the first four entries are used:
        support_x (n_way, k_shot, in_channels, num_points), support_y (n_way, k_shot, num_points),
        query_x (n_queries, in_channels, num_points), query_y (n_queries, num_points)."""
        support_x, support_y, query_x, query_y = (t.cuda() for t in self._augm.episode(data)[:4])
        self.model.train()
        query_logits, loss = self.model(support_x, support_y, query_x, query_y)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self.lr_scheduler.step()
        return loss, point_accuracy(query_logits.argmax(dim=1), query_y)

    def train_batch(self, datas, logger):
        """E episodes per optimiser step: ``datas`` is a list of what train() takes, all of one shape.  The E episodes go
        through ONE launch sequence (protonet_train.explicit_train_batch), their gradients are averaged -- over all ranks'
        episodes when torch.distributed is initialised: one flat all-reduce -- and there is ONE optimizer.step() and ONE
        lr_scheduler.step().  Returns a list with train()'s ``(loss, accuracy)`` for every episode: per episode what
        train() computes for it from the same weights and the same dropout seed.  May be interleaved with train() and
        test*() in any order (protonet_train.ProtoBatchTrainer says how the gradients stay apart)."""
        from .protonet_train import ProtoBatchTrainer
        b = self._augm.batch(self._batch(datas))
        if not self.model.use_attention:
            raise NotImplementedError("training with use_attention=False (the linear mapper) is not built: the training "
                                      "encoder (train_ops.encoder_forward) needs the attention learner")
        if self._batch_trainer is None:
            self._batch_trainer = ProtoBatchTrainer(self)
        loss, _, _, correct = self._batch_trainer.step(b)
        n = b.query_y.shape[1] * b.query_y.shape[2]
        return [(loss[e], c / n) for e, c in enumerate(correct.tolist())]  # (the step's one host read)

    def test(self, data, sampled_classes, step=None, path=None):
        [support_x, support_y, query_x, query_y, _, _, gt_support_y] = data
        self.model.eval()
        with torch.no_grad():
            logits, loss = self.model(support_x, support_y, query_x, query_y)
            pred = logits.argmax(dim=1)
        return pred, loss, point_accuracy(pred, query_y)
