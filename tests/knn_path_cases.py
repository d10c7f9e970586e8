"""The kNN case table: for every kernel configuration r3d_knn_topk_batched can launch (csrc/knn.hip: knn_choose), the
smallest call that reaches it -- shape, layout of x, debug switches -- and the r3d_debug_knn_path bit mask it CLAIMS.
tests/test_knn_paths_host.py holds every claim against the launcher's own decision (no GPU needed) and checks that no
leaf of that decision is left without a case; tests/test_gpu_knn_paths.py runs the cases against the C oracle, bit for bit.

The 256-tile line: the k <= 32 path takes 4 waves per tile and the bf16 passes when B * ceil(N / 32) > 256."""
from collections import namedtuple

import numpy as np

from r3dfsseg_amd import ops

SMALL, LARGE, INS = ops.KNN_PATH_SMALL, ops.KNN_PATH_LARGE, ops.KNN_PATH_INSERTION
FEW, SPLIT, BFA, FILTER = ops.KNN_PATH_FEW, ops.KNN_PATH_SPLIT, ops.KNN_PATH_BFA, ops.KNN_PATH_FILTER
ANY, LE16, FULL = ops.KNN_CHAN_ANY, ops.KNN_CHAN_LE16, ops.KNN_CHAN_FULL
DEFAULT = SMALL | BFA | FILTER | FULL  # the k <= 32 path at workload size

# layout of x: "plain" (B*N, C) contiguous; "ld65" buf[:, :C] of a (B*N, C + 1) buffer (ldx % 4 != 0); "off4" buf[:, 1:C + 1]
# of a (B*N, C + 4) buffer (rows 4 bytes off a 16-byte boundary); "x_cm": plain, and the channel-major copy handed over too;
# "no_x" (host only): x_cm alone.  fixed_scratch (host only): the call is r3d_knn_topk.
Case = namedtuple("Case", "name B C N k mode layout threshold filter status n_valid claim inputs gpu fixed_scratch")


def _c(name, B, C, N, claim, inputs=("plain", "dup"), k=20, mode="dgcnn", layout="plain", threshold=1, filter=1, status=False,
       n_valid=None, gpu=True, fixed_scratch=False):
    return Case(name, B, C, N, k, mode, layout, threshold, filter, status, n_valid, claim, tuple(inputs), gpu, fixed_scratch)


STRESS = ("offset", "tiny", "mixed_scale")

SMALL_CASES = (
    _c("A", 9, 64, 1024, DEFAULT, ("plain", "dup", "massive") + STRESS + ("nonfinite",)),
    _c("B", 9, 64, 1000, DEFAULT, ("plain", "dup", "massive") + STRESS),  # row tail: N % 32 = 8
    _c("C", 9, 64, 1024, SMALL | BFA | FULL, ("plain", "dup", "massive") + STRESS + ("nonfinite",), filter=0),
    _c("D", 9, 64, 1024, SMALL | FULL, threshold=0),
    _c("E1", 9, 64, 1024, SMALL | BFA | FULL, ("plain", "dup", "massive") + STRESS, layout="ld65"),
    _c("E2", 9, 64, 1024, SMALL | BFA | FULL, layout="off4"),
    _c("F1", 3, 64, 4096, DEFAULT, ("plain", "dup") + STRESS),  # grid.x = 128: the filter's bitmap is full
    _c("F2", 2, 64, 4128, SMALL | BFA | FULL),                  # grid.x = 129: no room for the bitmap
    _c("G", 9, 9, 1024, SMALL | LE16, ("plain", "dup", "massive")),
    _c("H", 9, 33, 1024, SMALL | ANY),
    _c("I1", 9, 64, 1024, DEFAULT, k=1),
    _c("I32", 9, 64, 1024, DEFAULT, k=32),
    _c("J", 9, 64, 1000, DEFAULT, layout="x_cm"),  # ldT = N = 1000, not the padded pitch
    _c("K", 9, 64, 1024, DEFAULT, mode="l2"),
    # fewer than 257 tiles: 8 waves per tile, fp32 passes
    _c("few9", 2, 9, 512, SMALL | FEW | LE16),
    _c("few64", 2, 64, 1024, SMALL | FEW | FULL),  # (the shape test_knn_bf16_threshold_pass_keeps_the_bits began with)
    _c("few33", 1, 33, 300, SMALL | FEW | ANY, k=7),
)

# SCORE_L2 with a status word, 192-wide features (the head's graphs); n_valid: one count per set, stride 1
LARGE_CASES = (
    _c("L1", 4, 192, 1400, LARGE | BFA | FULL, ("tail_nan", "tail_big"), k=201, mode="l2", status=True,
       n_valid=(1400, 1337, 700, 1001)),
    _c("L1f", 4, 192, 1400, LARGE | FULL, ("tail_nan",), k=201, mode="l2", status=True, n_valid=(1400, 1337, 700, 1001),
       threshold=0),
    _c("L2", 2, 192, 1500, LARGE | SPLIT | FULL, ("tail_nan", "tail_big", "tail_nan_offset"), k=201, mode="l2", status=True,
       n_valid=(1500, 1337)),
    _c("L3u", 4, 192, 1400, LARGE | BFA | FULL, ("ties400",), k=201, mode="l2", status=True, n_valid=(1400,) * 4),
    _c("L3s", 1, 192, 1400, LARGE | SPLIT | FULL, ("ties800",), k=201, mode="l2", status=True, n_valid=(1400,)),
    _c("L3i", 4, 192, 1400, INS | ops.KNN_REGS_4, ("ties400",), k=201, mode="l2", n_valid=(1400,) * 4),
    _c("L4a", 1, 100, 700, LARGE | SPLIT | ANY, ("plain",), k=65, mode="l2", status=True, n_valid=(700,)),
    _c("L4b", 1, 100, 700, LARGE | ANY, ("plain",), k=201, mode="l2", status=True, n_valid=(700,)),
    _c("ins64", 1, 64, 640, INS | ops.KNN_REGS_1, ("plain",), k=64),
    _c("ins65", 1, 100, 700, INS | ops.KNN_REGS_2, ("plain",), k=65, mode="l2", n_valid=(700,)),
)

# what only the host test asks: conditions no ops.knn call can produce
HOST_CASES = (
    _c("A_no_x", 9, 64, 1024, SMALL | FULL, layout="no_x", gpu=False),            # the pieces are cut from x: none, no bf16
    _c("A_topk", 9, 64, 1024, SMALL | FULL, gpu=False, fixed_scratch=True),       # r3d_knn_topk has no room for the pieces
    _c("L2_topk", 2, 192, 1500, LARGE | FULL, k=201, mode="l2", status=True, gpu=False, fixed_scratch=True),  # ... or the split
    _c("F1_edge", 2, 64, 4096, SMALL | FEW | FULL, gpu=False),                    # 256 tiles: still "few"
    _c("wide", 9, 128, 1024, INS | ops.KNN_REGS_1, gpu=False),                    # k <= 32 but C > 64, no status
    _c("wide_s", 9, 128, 1024, LARGE | BFA | FULL, status=True, gpu=False),       # ... with one: the large configuration
    _c("k33", 9, 64, 1024, INS | ops.KNN_REGS_1, k=33, gpu=False),
    _c("k129", 1, 192, 1400, INS | ops.KNN_REGS_4, k=129, gpu=False),
    _c("k128", 1, 192, 1400, INS | ops.KNN_REGS_2, k=128, gpu=False),
    _c("L_short", 1, 192, 803, LARGE | BFA | FULL, k=201, status=True, gpu=False),  # N < 4 k: a half would hold < 2 k candidates
)

ALL_CASES = SMALL_CASES + LARGE_CASES + HOST_CASES
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)


def path_args(case):
    """The arguments of r3d_debug_knn_path for a case, from its declared layout (the GPU tests pass what the tensors say)."""
    flags = (ops.KNN_FLAG_STATUS if case.status else 0) | (ops.KNN_FLAG_X_CM if case.layout in ("x_cm", "no_x") else 0)
    flags |= (ops.KNN_FLAG_NO_X if case.layout == "no_x" else 0) | (ops.KNN_FLAG_FIXED_SCRATCH if case.fixed_scratch else 0)
    ldx = {"ld65": case.C + 1, "off4": case.C + 4}.get(case.layout, case.C)
    return case.B, case.N, case.C, case.k, flags, ldx, 4 if case.layout == "off4" else 0


class switches:
    """The two debug switches set for a block, restored behind it."""

    def __init__(self, lib, threshold, filter):
        self.lib, self.want = lib, (threshold, filter)

    def __enter__(self):
        self.old = (self.lib.r3d_debug_set_knn_bf16_threshold(self.want[0]), self.lib.r3d_debug_set_knn_bf16_filter(self.want[1]))

    def __exit__(self, *exc):
        self.lib.r3d_debug_set_knn_bf16_threshold(self.old[0])
        self.lib.r3d_debug_set_knn_bf16_filter(self.old[1])


def leaves():
    """Every kernel configuration the launcher has, as bit masks, from the mask's fields alone: the product of the fields
    less what no kernel is instantiated for (csrc/knn.hip: the bf16 passes take whole 64-channel chunks, 4 waves and an
    unsplit candidate axis; the filter shares the threshold pass's pieces; the insertion kernel has its list length only)."""
    out = set()
    for chan in (ANY, LE16, FULL):
        for few in (0, FEW):
            out.add(SMALL | chan | few)
    out |= {SMALL | FULL | BFA, SMALL | FULL | BFA | FILTER}
    for chan in (ANY, FULL):
        for split in (0, SPLIT):
            out.add(LARGE | chan | split)
    out.add(LARGE | FULL | BFA)
    out |= {INS | r for r in (ops.KNN_REGS_1, ops.KNN_REGS_2, ops.KNN_REGS_4)}
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs
def small_input(kind, B, C, N):
    """(B, C, N) fp32 numpy.  The stress inputs are built as test_knn_bf16_threshold_pass_keeps_the_bits builds them, the
    duplicates as test_knn_duplicate_points_ties and test_knn_massive_duplicates_overflow_repair do."""
    if kind == "plain":
        return np.random.RandomState(1000 + B + C + N).randn(B, C, N).astype(np.float32)
    if kind == "dup":
        rs = np.random.RandomState(3)
        x = rs.randn(B, C, N).astype(np.float32)
        src, dst = rs.randint(0, N, 60), rs.randint(0, N, 60)
        x[:, :, dst] = x[:, :, src]
        return x
    if kind == "massive":  # 300 candidates tie at the best score: more than the 128 slots, the tile repair runs
        rs = np.random.RandomState(5)
        x = rs.randn(B, C, N).astype(np.float32)
        dup = rs.permutation(N)[:300]
        x[0][:, dup] = x[0][:, dup[:1]]
        return x
    rs = np.random.RandomState(17)
    x = rs.randn(B, C, N).astype(np.float32)
    if kind == "offset":
        x = x * 0.05 + 7.0
    elif kind == "tiny":
        x = x * 1e-18
    elif kind == "mixed_scale":
        x = x * np.logspace(-4, 3, C, dtype=np.float32)[None, :, None]
    elif kind == "nonfinite":
        x[0, :, 100] = np.inf
        x[1, 5, 300] = np.nan
    else:
        raise KeyError(kind)
    return x.astype(np.float32)


NONFINITE_QUERIES = ((0, 100), (1, 300))


def large_input(kind, B, C, N, n_valid):
    """(B, N, C) fp32 numpy, scaled as test_knn_l2_bitexact scales its features; rows at or beyond n_valid[b] poisoned."""
    rs = np.random.RandomState(31)
    if kind == "tail_nan_offset":  # the common offset of test_knn_l2_bf16_threshold_pass_with_large_norms
        X = np.stack([(rs.randn(N, C) * 0.07 + 1.0 + 0.1 * b).astype(np.float32) for b in range(B)])
    else:
        X = (rs.randn(B, N, C) * 0.2).astype(np.float32)
    if kind.startswith("ties"):  # identical rows in set 0, spread over the whole set
        rows = np.random.RandomState(37).permutation(N)[:int(kind[4:])]
        X[0, rows] = X[0, rows[0]]
    if kind.startswith("tail"):
        for b, n in enumerate(n_valid):
            X[b, n:] = np.nan if "nan" in kind else 3e38
    return X
