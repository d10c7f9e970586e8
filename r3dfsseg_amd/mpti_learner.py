"""Host-side mirror of the reference's models/mpti_learner.py::MPTILearner_V3.

Identical constructor, attributes (.model/.optimizer/.lr_scheduler) and train()/test()
signatures and return tuples (mpti_learner.py:50-102), so mpti_train_noise.py and
eval_noise.py run against it unchanged.  A checkpoint path of the literal string
"synthetic" initialises from r3dfsseg_amd.synthetic (no dataset/checkpoint files here).

The reference's schedule is one episode per call.  With ``args.episode_graphs = True`` (default off) train() / test()
capture the episode's launch sequence into ONE hipGraph on first use (shapes are fixed per run) and replay it afterwards
-- same kernels, same results, same return values (tests/test_gpu_graph.py); anything the graph cannot serve (other
shapes, a solver miss) falls back to the eager launches.  Measured at workload S: 86 episodes/s against 92 with eager
launches -- a single episode is a chain of ~440 dependent launches whose cost is the ~8 us from one kernel's end to the
next one's start, which a graph replay does not shorten; what the option buys is a free host thread (the replay costs
~0.3 ms of host time against ~9 ms of Python launch calls), e.g. for the data loader.  Throughput comes from episodes in
flight (dp_train.DPTrainer, episode_graph.EpisodeGraphs), not from this switch.
"""
import torch
from torch import optim

from .checkpoint_util import load_model_checkpoint, load_pretrain_checkpoint
from .fitted import FittedLearner
from .metrics import point_accuracy
from .mpti import MPTI_SelfAtten


class MPTILearner_V3(FittedLearner):
    def __init__(self, args, mode='train'):
        self.model = MPTI_SelfAtten(args)
        if not torch.cuda.is_available():
            raise RuntimeError("MPTILearner_V3 needs an MI355X: the forward pass has no CPU path")
        self.model.cuda()
        self.episode_graphs = bool(getattr(args, 'episode_graphs', False))
        from .augment import LearnerAugment
        self._augm = LearnerAugment(args)  # args.device_augm (+ args.pc_augm): --pc_augm on the device, train*() only
        self._trainer = None          # DPTrainer with one captured slot (train)
        self._batch_trainer = None    # DPTrainer(batch_size=E) behind train_batch
        self._batch_runner = None     # EpisodeBatchRunner behind test_batch
        self._eval_graphs = {}        # eval flag -> EpisodeGraphs with one captured slot (test)
        synthetic = 'synthetic' in (getattr(args, 'pretrain_checkpoint_path', None), getattr(args, 'model_checkpoint_path', None))
        if synthetic:
            from . import synthetic as S
            self.model.load_state_dict(S.make_state_dict(vars(args) if not isinstance(args, dict) else args))
        if mode == 'train':
            if args.use_attention:
                self.optimizer = torch.optim.Adam(
                    [{'params': self.model.encoder.parameters(), 'lr': 0.0001},
                     {'params': self.model.base_learner.parameters()},
                     {'params': self.model.att_learner.parameters()},
                     {'params': self.model.proj.parameters()}], lr=args.lr)
            self.lr_scheduler = optim.lr_scheduler.StepLR(self.optimizer, step_size=args.step_size, gamma=args.gamma)
            if not synthetic:
                if args.model_checkpoint_path is None:
                    self.model = load_pretrain_checkpoint(self.model, args.pretrain_checkpoint_path)
                else:
                    self.model, self.optimizer = load_model_checkpoint(self.model, args.model_checkpoint_path,
                                                                       optimizer=self.optimizer, mode='train')
        elif mode == 'test':
            if not synthetic:
                self.model = load_model_checkpoint(self.model, args.model_checkpoint_path, mode='test')
        else:
            raise ValueError('Wrong GraphLearner mode (%s)! Option:train/test' % mode)

    @staticmethod
    def _same_layout(tensors, example):
        return len(tensors) == len(example) and all(
            a.shape == b.shape and a.dtype == b.dtype for a, b in zip(tensors, example))

    def _train_graph(self, data, logger):
        """One episode through the captured launch sequence: forward + backward, status check, Adam (DPTrainer.step
        with one slot and one episode is exactly mpti_learner.py:60-72).  None when the graph cannot serve the call."""
        from .dp_train import DPTrainer
        if self._trainer is None:
            self._trainer = DPTrainer(self, n_slots=1, example=data)
        sl = self._trainer.graphs.slots[0]
        if not self._same_layout(data, sl.inputs):
            return None
        loss = self._trainer.step([data], logger=logger)
        if self._trainer.redone:  # the conservative eager pass ran instead: its results live in the eager buffers
            return self._tuple_from_eager(loss, data)
        lp, con, m0, m1, m2, m3 = sl.parts.unbind(0)
        accuracy = point_accuracy(sl.logits.argmax(dim=1), data[3])  # the step's host sync (mpti_learner.py:75)
        if logger is not None:
            v = sl.parts[2:].tolist()
            logger.cprint('after label propagation: QUERY prediction acc: {:.3f}, original_acc: {:.3f}'.format(v[0], v[1]))
            logger.cprint('after label propagation: clean_ratio_LP: {:.3f}, clean_ratio_original: {:.3f}'.format(v[2], v[3]))
        return (loss, lp.clone(), con.clone(), accuracy, m0.clone(), m1.clone(), m2.clone(), m3.clone())

    def _tuple_from_eager(self, loss, data):
        _, lp, con, logits, metrics = self._trainer.last_outputs[0]
        return (loss, lp, con, point_accuracy(logits.argmax(dim=1), data[3])) + tuple(metrics.unbind(0))

    def train(self, data, logger):
        data = self._augm.episode(data)  # once, here: the graph's input copy and a conservative redo see the same clouds
        if self.episode_graphs:
            out = self._train_graph(data, logger)
            if out is not None:
                return out
        [support_x, support_y, query_x, query_y, support_c, query_c, gt_support_y, gt_query_y, bg_pcd_x, bg_pcd_y,
         support_flag] = data
        self.model.train()
        from . import train_ops as T
        for lp_iters in (None, self.model.lp_max_iter):
            # an attempt's BatchNorm statistics are recorded and only the attempt that is kept updates the running
            # statistics (a discarded attempt would otherwise count the episode twice)
            with T.deferred_running_stats(self.model) as rec:
                (query_logits, lp_loss, contrastive_loss, query_acc_LP, query_acc_original, clean_ratio_LP_avg,
                 original_clean_ratio) = self.model(support_x, support_y, query_x, query_y, gt_support_y=gt_support_y,
                                                    gt_query_y=gt_query_y, train=True, logger=logger, bg_pcd_x=bg_pcd_x,
                                                    bg_pcd_y=bg_pcd_y, support_c=support_c, support_flag=support_flag,
                                                    lp_iters=lp_iters)
                loss = lp_loss + 0.1 * contrastive_loss
                self.optimizer.zero_grad()  # (its own gradients: the trainers bind .grad to their buckets at step time)
                loss.backward()
            # the CG solves (forward and adjoint) run on a launch budget and the 201-NN / FPS fast paths can report
            # overflow / time-out: never step Adam on an inexact gradient.  One host read per step, where the
            # reference synchronises anyway (`.item()` below, mpti_learner.py:75); a miss is redone once on the
            # conservative schedule (full budget, exact kernels).
            if self.model.lp_converged(backward=True):
                rec.apply(1)
                break
        else:
            raise RuntimeError("label propagation did not converge in %d CG iterations (forward or adjoint solve)"
                               % self.model.lp_max_iter)
        self.optimizer.step()
        self.lr_scheduler.step()
        query_pred = query_logits.argmax(dim=1)  # == softmax(dim=1).argmax(dim=1), mpti_learner.py:74
        accuracy = point_accuracy(query_pred, query_y)
        return (loss, lp_loss, contrastive_loss, accuracy, query_acc_LP, query_acc_original, clean_ratio_LP_avg,
                original_clean_ratio)

    def train_batch(self, datas, logger):
        """E episodes per optimiser step: ``datas`` is a list of the lists train() takes (dataloaders/loader.py:1666-1671),
        all of one shape.  The E episodes go through ONE launch sequence (batched.EpisodeBatchRunner: every kernel works on
        the whole batch, BatchNorm statistics stay per episode and getFeatures call), their gradients are averaged --
        over all ranks' episodes when torch.distributed is initialised: one all-reduce -- and Adam steps ONCE.  Returns
        a list with train()'s 8-tuple for every episode, so the driver loop keeps its per-episode bookkeeping
        (INTEGRATION.md shows the change to mpti_train_noise.py:57-98).  Against the reference's schedule (one Adam step
        per episode, mpti_learner.py:68-72) this is a larger-batch optimiser: per episode every number returned is what
        train() computes for it from the same weights (tests/test_gpu_batched.py); the step equals the eager schedule's
        accumulate-E-then-step (tests/test_gpu_learner_batch.py).  The step fails closed like train(): a solver miss redoes
        the episodes on the conservative schedule, and neither Adam nor the BatchNorm running statistics move on a step
        that could not be solved exactly."""
        from .dp_train import DPTrainer
        E = len(datas)
        if self._batch_trainer is None or self._batch_trainer.batch_size != E:
            self._batch_trainer = DPTrainer(self, batch_size=E, batch_graph=True)
        tr = self._batch_trainer
        if self._augm.on:  # once, before the step (its graph input copy, its redo): one launch over the batch's clouds
            from .batch import EpisodeBatch
            tr.step([self._augm.batch(EpisodeBatch.from_episodes(datas))], logger=logger)
        else:
            tr.step(datas, logger=logger)
        outs = tr.last_outputs
        qy = torch.stack([d[3] for d in datas], 0)
        logits = torch.stack([o[3] for o in outs], 0)
        acc = torch.eq(logits.argmax(dim=2), qy).float().mean(dim=(1, 2))
        host = torch.cat((acc[:, None], torch.stack([o[4] for o in outs], 0).to(acc.dtype)), 1).tolist()  # the step's host read
        res = []
        for e, o in enumerate(outs):
            accuracy, m = host[e][0], host[e][1:]
            if logger is not None:
                logger.cprint('after label propagation: QUERY prediction acc: {:.3f}, original_acc: {:.3f}'.format(m[0], m[1]))
                logger.cprint('after label propagation: clean_ratio_LP: {:.3f}, clean_ratio_original: {:.3f}'.format(m[2], m[3]))
            res.append((o[0], o[1], o[2], accuracy) + tuple(o[4].unbind(0)))
        return res

    def test_batch(self, datas, sampled_classes=None, step=None, path=None, eval=False):
        """test() for E episodes of one shape in ONE launch sequence (MPTI_SelfAtten.forward_episodes): a list of
        (pred (n_q, N), loss, accuracy), per episode what test() returns for it.  A batch in which any system missed its CG
        launch budget (or overflowed the 201-NN survivor buffer) is redone episode by episode through test()."""
        from . import dist as D
        from .batch import EpisodeBatch
        self.model.eval()
        D.warn_rank_local_stats(self.model, 'evaluation')
        b = datas if isinstance(datas, EpisodeBatch) else EpisodeBatch.from_episodes(datas)
        with torch.no_grad():
            logits, loss = self.model.forward_episodes(b, eval=eval)
            pred = logits.argmax(dim=2)
            acc = torch.eq(pred, b.query_y).float().mean(dim=(1, 2)).tolist()
        if not self.model.lp_converged():
            return [self.test(b.episode(e)[:4] + [None, None, b.gt_support_y[e]], sampled_classes, step, path, eval)
                    for e in range(b.E)]
        return [(pred[e], loss[e], acc[e]) for e in range(b.E)]

    def predict(self, query_x, query_y=None, fitted=None):
        """fitted.FittedLearner.predict, following test() on a miss: a call whose budgeted schedule did not converge (or
        overflowed the 201-NN survivor buffer) is redone with lp_iters=model.lp_max_iter; it raises if that fails too."""
        fitted = self._fitted_or_raise(fitted)
        self.model.eval()
        from . import dist as D
        D.warn_rank_local_stats(self.model, 'evaluation')
        query_x = query_x.cuda()
        query_y = query_y.cuda() if query_y is not None else None
        with torch.no_grad():
            pred, loss, correct = self._exact(lambda lp_iters: self._predict_once(fitted, query_x, query_y, lp_iters))[0]
        return self._predict_result(query_x, pred, loss, correct)

    def _exact(self, run):
        """The redo rule of every inference launch: run(lp_iters=None), the budgeted schedule; a launch that did not
        converge (or overflowed the 201-NN survivor buffer, or timed out in the FPS) is redone as a whole on the
        conservative one, run(model.lp_max_iter); it raises if that misses too.  -> (what run returned, redone)."""
        out = run(None)
        if self.model.lp_converged():
            return out, False
        out = run(self.model.lp_max_iter)
        if not self.model.lp_converged():
            raise RuntimeError("label propagation did not converge in %d CG iterations" % self.model.lp_max_iter)
        return out, True

    def _scene_launch(self, fitted, query_x):
        """One launch of predict_scene under predict()'s rule (_exact) -> (logits, redone)."""
        return self._exact(lambda lp_iters: self.model._predict_groups(fitted, query_x, None, lp_iters=lp_iters)[0])

    def _scene_launch_sets(self, fits, query_x):
        """_scene_launch for K support sets: lp_converged() speaks for the K * G systems of the launch, and a miss redoes
        all of them."""
        return self._exact(lambda lp_iters: self.model._predict_groups_sets(fits, query_x, lp_iters=lp_iters).reshape(
            query_x.shape[0], -1, query_x.shape[-1]))

    def _test_graph(self, data, eval):
        from .episode_graph import EpisodeGraphs
        episode = list(data[:4])
        g = self._eval_graphs.get(bool(eval))
        if g is None:
            self.model.eval()
            g = self._eval_graphs[bool(eval)] = EpisodeGraphs(self.model, episode, n_slots=1, train=False, eval_flag=bool(eval))
        sl = g.slots[0]
        if not self._same_layout(episode, sl.inputs):
            return None
        loss = g.run([episode])
        bad, overflow, _, _ = g.step_status()  # host wait: the reference synchronises here too (mpti_learner.py:99)
        if bad or overflow:
            return None                          # the eager path below redoes the episode on the conservative schedule
        pred = sl.logits.argmax(dim=1)
        return pred, loss.clone(), point_accuracy(pred, data[3])

    def test(self, data, sampled_classes, step=None, path=None, eval=False):
        if self.episode_graphs:
            out = self._test_graph(data, eval)
            if out is not None:
                return out
        [support_x, support_y, query_x, query_y, _, _, gt_support_y] = data
        self.model.eval()
        from . import dist as D
        D.warn_rank_local_stats(self.model, 'evaluation')

        def run(lp_iters):
            logits, loss = self.model(support_x, support_y, query_x, query_y, gt_support_y=gt_support_y,
                                      sampled_classes=sampled_classes, step=step, path=path, support_flag=None,
                                      eval=eval, lp_iters=lp_iters)
            pred = logits.argmax(dim=1)
            return pred, loss, point_accuracy(pred, query_y)

        with torch.no_grad():
            return self._exact(run)[0]  # (a CG launch budget too small for this episode: redone in full)
