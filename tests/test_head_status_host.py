"""ops.head_status, the one reading of a head launch's status words (CG converged, adjoint converged, 201-NN survivor
overflow, FPS time-out), on hand-made CPU tensors; and that the three product readers have no reading of their own."""
import inspect

import pytest
import torch

from r3dfsseg_amd import ops
from r3dfsseg_amd.batched import EpisodeBatchRunner
from r3dfsseg_amd.episode_graph import EpisodeGraphs
from r3dfsseg_amd.mpti import MPTI_SelfAtten

ITERS = {1: [17], 3: [17, 31, 5]}  # unequal CG iteration counts


def _words(E):
    """Status words of E systems after a launch in which nothing went wrong."""
    stats = torch.tensor([[1, it] for it in ITERS[E]], dtype=torch.int32)
    desc = torch.arange(E * 32, dtype=torch.int32).reshape(E, 32) + 1  # every other descriptor word is in use
    desc[:, ops.HD_FPS_TIMEOUT] = 0
    stats_bwd = torch.tensor([[1, 40 + e] for e in range(E)], dtype=torch.int32)
    return stats, desc, torch.zeros(1, dtype=torch.int32), stats_bwd


def _status(stats, desc, knn, stats_bwd=None):
    out = ops.head_status(stats, desc, knn, stats_bwd)
    assert out.dtype == torch.int32 and out.shape == (4,)
    return out.tolist()


@pytest.mark.parametrize("E", [1, 3])
def test_all_good(E):
    stats, desc, knn, bwd = _words(E)
    want = [0, 0, sum(ITERS[E]), max(ITERS[E])]
    assert _status(stats, desc, knn) == want
    assert _status(stats, desc, knn, bwd) == want  # the adjoint's iteration counts are not part of the sum or the maximum


@pytest.mark.parametrize("E", [1, 3])
def test_one_forward_solve_not_converged(E):
    stats, desc, knn, bwd = _words(E)
    stats[E - 1, 0] = 0
    assert _status(stats, desc, knn) == [1, 0, sum(ITERS[E]), max(ITERS[E])]
    assert _status(stats, desc, knn, bwd) == [1, 0, sum(ITERS[E]), max(ITERS[E])]


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("word", [1, 7])
def test_an_fps_time_out_counts_once_whatever_the_word(E, word):
    stats, desc, knn, _ = _words(E)
    desc[0, ops.HD_FPS_TIMEOUT] = word
    assert _status(stats, desc, knn)[:2] == [1, 0]


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("word", [1, 2, 3])
def test_knn_overflow_is_a_flag(E, word):
    stats, desc, knn, _ = _words(E)
    knn[0] = word
    assert _status(stats, desc, knn)[:2] == [0, 1]


@pytest.mark.parametrize("E", [1, 3])
def test_the_adjoint_counts_only_when_asked(E):
    stats, desc, knn, bwd = _words(E)
    bwd[E - 1, 0] = 0
    assert _status(stats, desc, knn)[:2] == [0, 0]
    assert _status(stats, desc, knn, bwd)[:2] == [1, 0]


@pytest.mark.parametrize("E", [1, 3])
def test_one_system_that_fails_three_ways_counts_three(E):
    """Forward miss + adjoint miss + FPS time-out of ONE system: 3, the sum EpisodeBatchRunner's counters have always held."""
    stats, desc, knn, bwd = _words(E)
    e = E - 1
    stats[e, 0], bwd[e, 0], desc[e, ops.HD_FPS_TIMEOUT] = 0, 0, 1
    assert _status(stats, desc, knn, bwd)[:2] == [3, 0]
    assert _status(stats, desc, knn)[:2] == [2, 0]


def test_every_system_of_a_batch_is_counted():
    stats, desc, knn, bwd = _words(3)
    stats[:, 0] = 0
    bwd[1:, 0] = 0
    desc[2, ops.HD_FPS_TIMEOUT] = 5
    knn[0] = 1
    assert _status(stats, desc, knn, bwd) == [3 + 2 + 1, 1, 17 + 31 + 5, 31]


def test_iterations_of_a_non_contiguous_view():
    """The words as the head buffers hand them over: columns of (E, 2) and (E, 32) arrays."""
    stats, desc, knn, _ = _words(3)
    stats[:, 1] = torch.tensor([9, 2, 200], dtype=torch.int32)
    assert _status(stats, desc, knn)[2:] == [211, 200]


@pytest.mark.parametrize("reader", [MPTI_SelfAtten.lp_converged, EpisodeBatchRunner._count, EpisodeGraphs._run_once])
def test_the_readers_have_no_reading_of_their_own(reader):
    """Adam steps, or does not, on what these three return: each asks HeadBuffers.status and compares no status word itself."""
    src = inspect.getsource(reader)
    assert ".status(" in src
    for word in ("stats", "knn_status", "HD_FPS_TIMEOUT", "desc"):
        assert word not in src, "%s reads %s itself" % (reader.__qualname__, word)
    src = inspect.getsource(ops.HeadBuffers.status)
    assert "head_status(self.stats, self.desc, self.knn_status" in src
