"""The learner eval_noise.py:120-121 asks for under --phase protoeval (it names a `ProtoNet_learner` the reference never
defines): ProtoNet_Contrast -- ProtoNet + clean-shot detection, "protonet+CCNS+MDNS" -- on a ProtoNet checkpoint.
Evaluation only: test() / test_batch() with the return values of ProtoLearner's."""
import torch

from .checkpoint_util import load_model_checkpoint
from .metrics import point_accuracy
from .proto_learner import ProtoEvalBatch
from .protonet import ProtoNet_Contrast


class ProtoContrastLearner(ProtoEvalBatch):
    def __init__(self, args, mode='test'):
        if mode == 'train':
            raise NotImplementedError("ProtoContrastLearner evaluates: ProtoNet_Contrast is a test-time method on a ProtoNet "
                                      "checkpoint (train it with ProtoLearner); the reference has no learner for its "
                                      "train=True branch")
        if mode != 'test':
            raise ValueError('Wrong ProtoContrastLearner mode (%s)! Option:test' % mode)
        self.model = ProtoNet_Contrast(args)
        if not torch.cuda.is_available():
            raise RuntimeError("ProtoContrastLearner needs an MI355X: the forward pass has no CPU path")
        self.model.cuda()
        if getattr(args, 'model_checkpoint_path', None) == 'synthetic':
            from . import synthetic as S
            self.model.load_state_dict(S.make_state_dict(vars(args)))
        else:  # non-strict, as the reference's loader: a ProtoNet checkpoint has no proj.*, which evaluation never reads
            self.model = load_model_checkpoint(self.model, args.model_checkpoint_path, mode='test')

    # test_batch: ProtoEvalBatch's (forward_episodes on self.model: the detection runs inside the one launch sequence)

    def test(self, data, sampled_classes, step=None, path=None, eval=False):
        """One episode (eval_noise.py:91 passes step, path and eval; the detection runs whatever `eval` says, as in the
        reference's forward).  Returns (pred (n_q, N), loss, accuracy)."""
        support_x, support_y, query_x, query_y = data[:4]
        self.model.eval()
        with torch.no_grad():
            logits, loss = self.model(support_x, support_y, query_x, query_y)
            pred = logits.argmax(dim=1)
        return pred, loss, point_accuracy(pred, query_y)
