"""What a frozen launch sequence needs (episode_graph.EpisodeGraphs, batched.BatchGraph): state that the warm-up and capture
passes leave as they found it, the capture itself, and a CG launch budget that follows the iteration counts."""
import contextlib
import ctypes

import torch

from . import _lib


@contextlib.contextmanager
def preserved(model, extra=()):
    """Warm-up and capture passes are not episodes of any step: the model's buffers (BatchNorm running statistics) and the
    `extra` tensors they add into (a gradient sink, status counters) come back as they were, also when the capture fails."""
    saved = [(t, t.clone()) for t in [b for _, b in model.named_buffers()] + list(extra)]
    try:
        yield
    finally:
        with torch.no_grad():
            for t, c in saved:
                t.copy_(c)


def capture(fn, stream, warmup=2, capture_stream=None):
    """fn()'s launches as an instantiated hipGraph.  The eager warm-up passes on `stream` come first: allocations, head
    buffers, lazily initialised library state.  capture_stream: the stream the capture runs on (None: torch's own)."""
    cur = torch.cuda.current_stream()
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
    cur.wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)  # the hipGraph_t stays: its nodes are enabled / disabled later
    # thread-local capture mode: only this thread launches into the capture (no autograd engine threads), while other
    # threads -- e.g. the RCCL watchdog of torch.distributed polling its events -- must stay free to call the HIP runtime
    with torch.cuda.graph(graph, stream=capture_stream, capture_error_mode="thread_local"):
        fn()
    graph.instantiate()
    return graph


class LpBudget:
    """The CG iterations of a captured sequence: `captured` of them are frozen into the graph, of which the first `active`
    stay enabled (r3d_graph_set_lp_budget: a disabled kernel node is an empty node)."""

    def __init__(self, captured):
        self.captured = self.active = int(captured)
        self._mx_decay = 0  # slowly decaying maximum of the iteration counts seen

    @staticmethod
    def budget_for(mx):
        """Enabled CG iterations for an observed maximum of `mx`: half as many again plus 8, rounded up to 8, at least 24
        (convergence is detected inside the last productive launch, so nothing extra is needed for the test itself)."""
        return max(24, 8 * ((mx + mx // 2 + 8 + 7) // 8))

    def target(self, bad, mx, adaptive=True):
        """The budget of the next replays after a finished run with `bad` misses and `mx` iterations at most: a miss goes
        back to everything that was captured; otherwise the budget follows a decaying maximum, so it can shrink again."""
        budget = self.active
        if bad:
            self._mx_decay = max(self._mx_decay, mx)
            budget = self.captured
        elif adaptive and mx > 0:
            self._mx_decay = max(mx, self._mx_decay - max(1, self._mx_decay // 16))
            budget = self.budget_for(self._mx_decay)
        return max(1, min(budget, self.captured))

    def apply(self, graphs, budget, sync, force=False):
        """Enable the CG kernel nodes of the first `budget` iterations in every graph, disable the rest.  sync(i) runs before
        graphs[i] is edited (never edit an executable graph in flight); force: also when the budget does not change."""
        budget = max(1, min(int(budget), self.captured))
        if budget == self.active and not force:
            return
        for i, g in enumerate(graphs):
            sync(i)
            n_cg = ctypes.c_int(0)
            _lib.check(_lib.load().r3d_graph_set_lp_budget(ctypes.c_void_p(g.raw_cuda_graph()), ctypes.c_void_p(g.raw_cuda_graph_exec()),
                                                   budget, ctypes.byref(n_cg)))
            assert n_cg.value > 0, "no CG nodes found in the captured sequence"
        self.active = budget
