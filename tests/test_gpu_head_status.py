"""The status words of a real head launch through the product's readers: MPTI_SelfAtten.lp_converged and
EpisodeBatchRunner._count both go through ops.head_status (tests/test_head_status_host.py has its arithmetic), here on the
head buffers an eval forward left behind, one word poked at a time.  Only status words are written; no library kernel runs
on a poked buffer."""
from types import SimpleNamespace

import pytest
import torch

from r3dfsseg_amd import synthetic as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    """The smallest eval episode of tests/test_gpu_head.py, its synthetic weights, one runner around the model."""
    from r3dfsseg_amd import _lib, ops
    from r3dfsseg_amd.batched import EpisodeBatchRunner
    from r3dfsseg_amd.mpti import MPTI_SelfAtten
    _lib.load()
    cfg = S.make_cfg(n_way=2, k_shot=1, pc_npts=512)
    m = MPTI_SelfAtten(SimpleNamespace(**cfg))
    m.load_state_dict(S.make_state_dict(cfg, 123))
    m.cuda().eval()
    data, _ = S.make_episode(cfg, 1)
    return ops, m, EpisodeBatchRunner(m), [t.cuda() for t in data[:4]]


def _counted(runner, backward):
    runner.begin_step()
    runner._count(backward)
    return runner.step_status()


def _check(ops, m, runner, sys):
    """The truth table of the four words, poked in system `sys` of the head buffers the last forward used."""
    hb = m._head[1]
    hb.stats_bwd[:, 0] = 1  # as after an adjoint solve that converged (an eval forward leaves the zeros it was made with)
    its = hb.stats[:, 1].tolist()
    assert m.lp_converged() and m.lp_converged(backward=True)
    assert _counted(runner, False) == _counted(runner, True) == (0, 0, sum(its), max(its))
    # (word, value, lp_converged(), lp_converged(backward=True), bad without / with the adjoint, overflow)
    table = [(hb.stats[sys, 0:1], 0, False, False, 1, 1, 0),
             (hb.desc[sys, ops.HD_FPS_TIMEOUT:ops.HD_FPS_TIMEOUT + 1], 1, False, False, 1, 1, 0),
             (hb.knn_status, 2, False, False, 0, 0, 1),
             (hb.stats_bwd[sys, 0:1], 0, True, False, 0, 1, 0)]
    for i, (word, value, fwd, bwd, bad_f, bad_b, ovf) in enumerate(table):
        saved = word.clone()
        word.fill_(value)
        try:
            assert m.lp_converged() is fwd and m.lp_converged(backward=True) is bwd, i
            assert hb.status(False)[:2].tolist() == [bad_f, ovf] and hb.status(True)[:2].tolist() == [bad_b, ovf], i
            assert _counted(runner, False) == (bad_f, ovf, sum(its), max(its)), i
            assert _counted(runner, True) == (bad_b, ovf, sum(its), max(its)), i
        finally:
            word.copy_(saved)
        assert m.lp_converged() and m.lp_converged(backward=True), i
    # every word of the system at once: 3 from it alone, and the counters add over calls
    hb.stats[sys, 0], hb.stats_bwd[sys, 0], hb.desc[sys, ops.HD_FPS_TIMEOUT] = 0, 0, 7
    runner.begin_step()
    runner._count(True)
    runner._count(False)
    assert runner.step_status() == (3 + 2, 0, 2 * sum(its), max(its))
    hb.stats[sys, 0], hb.stats_bwd[sys, 0], hb.desc[sys, ops.HD_FPS_TIMEOUT] = 1, 1, 0
    assert m.lp_converged(backward=True)


def test_one_episode(setup):
    ops, m, runner, (sx, sy, qx, qy) = setup
    with torch.no_grad():
        m(sx, sy, qx, qy, lp_iters=m.lp_max_iter)
    hb = m._head[1]
    assert hb.E == 1 and hb.stats.shape == (1, 2) and hb.desc.shape == (1, 32) and hb.stats_bwd.shape == (1, 2)
    _check(ops, m, runner, 0)


def test_a_batch_of_two_system_1_poked(setup):
    from r3dfsseg_amd.batch import EpisodeBatch
    ops, m, runner, ep = setup
    with torch.no_grad():
        m.forward_episodes(EpisodeBatch.from_episodes([ep, ep]), lp_iters=m.lp_max_iter)
    hb = m._head[1]
    assert hb.E == 2 and hb.stats.shape == (2, 2)
    _check(ops, m, runner, 1)
