"""The kNN case table (tests/knn_path_cases.py) against the launcher's own decision, without a GPU: r3d_debug_knn_path is
the host function r3d_knn_topk_batched branches on (csrc/knn.hip: knn_choose), so a claim that holds here is the kernel
configuration the GPU test of that case runs -- and a threshold moved in knn.hip fails here, not silently there."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_path_cases as KC  # noqa: E402

from r3dfsseg_amd import _lib, ops  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from r3dfsseg_amd import build
    build.build()
    return _lib.load()


def _describe(mask):
    if mask < 0:
        return "refused"
    names = [("small", "large", "insertion", "?")[mask & ops.KNN_PATH_MASK]]
    names += [n for bit, n in ((ops.KNN_PATH_FEW, "few"), (ops.KNN_PATH_SPLIT, "split"), (ops.KNN_PATH_BFA, "bfa"),
                               (ops.KNN_PATH_FILTER, "filter")) if mask & bit]
    names.append(("chan=any", "chan<=16", "chan=full", "chan=?")[(mask & ops.KNN_PATH_CHAN_MASK) >> ops.KNN_PATH_CHAN_SHIFT])
    names.append("regs=%d" % ((mask & ops.KNN_PATH_REGS_MASK) >> ops.KNN_PATH_REGS_SHIFT))
    return " ".join(names)


@pytest.mark.parametrize("case", KC.ALL_CASES, ids=lambda c: c.name)
def test_case_reaches_the_path_it_claims(lib, case):
    with KC.switches(lib, case.threshold, case.filter):
        got = lib.r3d_debug_knn_path(*KC.path_args(case))
    assert got == case.claim, "%s: claimed %s, the launcher takes %s" % (case.name, _describe(case.claim), _describe(got))


def test_every_leaf_of_the_launcher_is_claimed_and_on_the_gpu(lib):
    """Every kernel configuration (the leaves: KC.leaves(), from the mask's fields) is claimed by a case that runs on the
    GPU; no case claims anything else; and the launcher, swept over shapes, layouts and switch settings, reaches exactly
    these leaves -- a configuration added to knn.hip without a case fails here."""
    leaves = KC.leaves()
    assert len(leaves) == 16
    claimed = {c.claim for c in KC.ALL_CASES if c.gpu}
    assert claimed == leaves, sorted(_describe(m) for m in claimed ^ leaves)
    assert {c.claim for c in KC.ALL_CASES} <= leaves
    reached = set()
    shapes = [(B, N, C, k) for B in (1, 2, 9) for N in (300, 1024, 4096, 4128) for C in (9, 16, 17, 64, 100, 128, 192)
              for k in (1, 20, 32, 33, 64, 65, 128, 129, 256)]
    for thr, fil in itertools.product((0, 1), (0, 1)):
        with KC.switches(lib, thr, fil):
            for (B, N, C, k), flags, (pad, mis) in itertools.product(shapes, range(16), ((0, 0), (1, 0), (4, 4))):
                if flags & ops.KNN_FLAG_NO_X and not flags & ops.KNN_FLAG_X_CM:
                    continue
                reached.add(lib.r3d_debug_knn_path(B, N, C, k, flags, C + pad, mis))
    assert reached == leaves, sorted(_describe(m) for m in reached ^ leaves)


def test_switches_and_layout_only_move_the_bf16_bits(lib):
    """The switches, the row pitch and the alignment of x select among the bf16 forms and nothing else; a refused shape
    is refused."""
    keep = ~(ops.KNN_PATH_BFA | ops.KNN_PATH_FILTER)
    for case in KC.ALL_CASES:
        B, N, C, k, flags, ldx, mis = KC.path_args(case)
        seen = set()
        for thr, fil in itertools.product((0, 1), (0, 1)):
            with KC.switches(lib, thr, fil):
                for pad, m in ((0, 0), (1, 0), (4, 4), (4, 8)):
                    seen.add(lib.r3d_debug_knn_path(B, N, C, k, flags, C + pad, m) & keep)
        assert len(seen) == 1, (case.name, [_describe(m) for m in seen])
    assert lib.r3d_debug_knn_path(1, 64, 9, 65, 0, 9, 0) == -1   # k > N
    assert lib.r3d_debug_knn_path(1, 1024, 9, 257, 0, 9, 0) == -1
    assert lib.r3d_debug_knn_path(0, 1024, 9, 20, 0, 9, 0) == -1
