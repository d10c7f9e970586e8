"""The cases of tests/test_gpu_gemm_kernels.py, each with the kernel path it claims; tests/test_gemm_ref_host.py holds every
claim to r3d_debug_pointwise_path / r3d_debug_gemm_tn_plan (the host functions the launchers branch on) without a GPU, and
checks that the tables name every path, every epilogue variant and every edge value the module promises.

Point-wise paths (include/r3d.h): 0 = r3d_pointwise_gemm_kernel (fp32 core: 64 x 64 tile, K-steps of 32, masked K tail),
1 = r3d_pointwise_gemm_bx3_kernel (bf16 x 3, W cut per tile: 256-row tile of four 64-row waves, 64 / 128 columns),
2 = r3d_pointwise_gemm_bx3p_kernel (bf16 x 3, packed W: 128-row tile of four 32-row waves).  The claimed path holds under
r3d_set_matrix_arith(1) and the case's r3d_debug_set_gemm_bx3 mask (7 = default, 3 = no packed kernel); under arithmetic 0
every case runs on path 0."""
from collections import namedtuple

PW = namedtuple("PW", "name M K Co mask path what")

# ---- A: one axis sweeps, the two others sit at an edge value ---------------------------------------------------------
FP32_M, FP32_CO, FP32_K = (1, 63, 64, 65, 129), (1, 31, 63, 64, 65), (1, 9, 31, 32, 33, 64, 65, 100)
BX3_M, BX3_M_MASK3 = (64, 65, 127, 128, 129, 255), (256, 257, 511, 513)
BX3P_M = (256, 257, 281, 287, 288, 289, 383, 384, 385)
BF_CO, BF_K = (32, 36, 60, 64, 68, 96, 128, 132, 160, 192), (32, 64, 96, 160)


def _sweeps():
    out = []
    # fp32 kernel: Co = 65 (not a multiple of 4) keeps the bf16 forms away under either arithmetic
    out += [PW("fp32 M=%d" % m, m, 33, 65, 7, 0, "rows on both sides of the 64-row tile, one row, a third tile; K = 33 and "
               "Co = 65 one beyond a step / a tile") for m in FP32_M]
    out += [PW("fp32 Co=%d" % c, 65, 33, c, 7, 0, "columns on both sides of the 32-column wave and the 64-column tile; "
               "M = 65, K = 33") for c in FP32_CO if c != 64]
    out += [PW("fp32 Co=64", 65, 33, 64, 7, 0, "a full column tile (K = 33 keeps it on the fp32 kernel); M = 65")]
    out += [PW("fp32 K=%d" % k, 65, k, 65, 7, 0, "K on both sides of one and two K-steps of 32, a masked tail of 1, 4, 9, 31; "
               "M = 65, Co = 65") for k in FP32_K]
    # bf16 x 3, W cut per tile: M < 256 under the default mask, M >= 256 under mask 3
    out += [PW("bx3 M=%d" % m, m, 96, 132, 7, 1, "rows on both sides of the 64-row wave inside the 256-row tile (waves without a "
               "row); K = 96 (three steps), Co = 132 (a 4-column tail in a second 128-column tile)") for m in BX3_M]
    out += [PW("bx3 M=%d mask 3" % m, m, 96, 132, 3, 1, "rows on both sides of the 256-row tile and of two tiles; K = 96, Co = 132")
            for m in BX3_M_MASK3]
    out += [PW("bx3 Co=%d" % c, 129, 96, c, 7, 1, "column tails inside the 64-column (Co <= 64) and the 128-column tile; M = 129 "
               "(a wave of one row), K = 96") for c in BF_CO]
    out += [PW("bx3 K=%d" % k, 129, k, 132, 7, 1, "one K-step (kn clamped onto itself), two, an odd count (3, 5); M = 129, Co = 132")
            for k in BF_K]
    # bf16 x 3, packed W
    out += [PW("bx3p M=%d" % m, m, 96, 132, 7, 2, "a last tile of one row (257, 385), a partial group of 8 rows (281, 287), waves "
               "without a row, full tiles (256, 384); K = 96, Co = 132") for m in BX3P_M]
    out += [PW("bx3p Co=%d" % c, 289, 96, c, 7, 2, "column tails inside the packed 64- and 128-column tile; M = 289 (wave 1 of the "
               "third tile has one row), K = 96") for c in BF_CO]
    out += [PW("bx3p K=%d" % k, 289, k, 132, 7, 2, "one K-step, two, an odd count; M = 289, Co = 132") for k in BF_K]
    return out


SWEEPS = _sweeps()


def pw_geometry(c):
    """-> (ldx, x_col0, ldo, out_col0): X is columns [4, 4 + K) of a wide matrix of K + 8, Out columns [4, 4 + Co) of one of
    Co + 8 rounded up to a multiple of 4 -- 16-byte aligned slices whenever the shape allows a bf16 form."""
    return c.K + 8, 4, c.Co + 8 + (-c.Co) % 4, 4


# the scratch of the packed kernel: 4 MiB at first, so Co K > 699 050 makes it grow (run on a stream of its own)
GROW_SMALL, GROW_LARGE = PW("bx3p scratch small", 256, 64, 64, 7, 2, "first call of a stream: the scratch is made"), \
    PW("bx3p scratch grows", 256, 704, 1024, 7, 2, "1024 x 704 x 6 B = 4.3 MB right after the small one: the scratch grows")

# ---- B: the epilogue, one full-tile and one tail shape per kernel -----------------------------------------------------
EPILOGUE = [
    PW("fp32 full", 64, 32, 64, 0, 0, "one full 64 x 64 tile, one K-step (mask 0: the bf16 forms are off)"),
    PW("fp32 tail", 65, 33, 65, 7, 0, "every axis one beyond"),
    PW("bx3 full", 256, 64, 128, 3, 1, "one full 256 x 128 tile"),
    PW("bx3 tail", 129, 96, 36, 7, 1, "a wave of one row, two waves without, a 4-column tail in a 64-column tile"),
    PW("bx3p full", 256, 64, 128, 7, 2, "two full 128 x 128 tiles: every wave takes a FULL variant"),
    PW("bx3p tail", 281, 96, 132, 7, 2, "FULL waves (tiles 0, 1, columns 0..127) beside tail waves: 25 rows, no row, 4 columns"),
]
ACTS = (0, 1, 2)
AFFINE = ((0, 0), (1, 0), (0, 1), (1, 1))  # (scale given, shift given)


def packed_variants(M, Co, plain, stats):
    """The (PLAIN, STATS, FULL) epilogue variants the waves of r3d_pointwise_gemm_bx3p_kernel take on an (M, Co) output:
    restated from the kernel's wave-uniform branches (full = the wave's 32 rows and the tile's columns all inside)."""
    bn = 128 if Co > 64 else 64
    seen = set()
    for tile_m in range(-(-M // 128)):
        for w in range(4):
            mw = 128 * tile_m + 32 * w
            for n0 in range(0, -(-Co // bn) * bn, bn):
                full = mw + 32 <= M and n0 + bn <= Co
                if plain:
                    seen.add((True, bool(stats), full))
                else:
                    seen.add((False, bool(stats), False if stats else full))
    return seen


# the six variants the ABI reaches (non-PLAIN with STATS is one generic variant no entry point launches)
PACKED_VARIANTS = {(True, True, True), (True, True, False), (True, False, True), (True, False, False),
                   (False, False, True), (False, False, False)}

# ---- C: the fall-back rules: the base shape (256, 64, 64) takes path 2; one rule is broken per case ------------------
FB = namedtuple("FB", "name M K Co ldx_pad ldo_pad x_off w_off out_off rule")
# ldx = K + 8 + ldx_pad with X at column 4 + x_off of the wide matrix, ldo likewise; w_off floats into its aligned buffer
FALLBACKS = [
    FB("K=48", 256, 48, 64, 0, 0, 0, 0, 0, "K % 32 != 0"),
    FB("K=16", 256, 16, 64, 0, 0, 0, 0, 0, "K < 32"),
    FB("Co=28", 256, 64, 28, 0, 0, 0, 0, 0, "Co < 32"),
    FB("Co=66", 256, 64, 66, 0, 2, 0, 0, 0, "Co % 4 != 0"),
    FB("M=63", 63, 64, 64, 0, 0, 0, 0, 0, "M < 64"),
    FB("ldx=73", 256, 64, 64, 1, 0, 0, 0, 0, "ldx % 4 != 0"),
    FB("X+4B", 256, 64, 64, 0, 0, 1, 0, 0, "X 4 bytes off 16"),
    FB("W+4B", 256, 64, 64, 0, 0, 0, 1, 0, "W 4 bytes off 16"),
    FB("Out+4B", 256, 64, 64, 0, 0, 0, 0, 1, "Out 4 bytes off 16"),
    FB("ldo=73", 256, 64, 64, 0, 1, 0, 0, 0, "ldo % 4 != 0"),
]
FALLBACK_RULES = ("K % 32 != 0", "Co < 32", "Co % 4 != 0", "M < 64", "ldx % 4 != 0", "X 4 bytes off 16", "W 4 bytes off 16",
                  "Out 4 bytes off 16", "ldo % 4 != 0")


def fb_geometry(c):
    """-> (ldx, x_col0, ldo, out_col0) of a fall-back case."""
    return c.K + 8 + c.ldx_pad, 4 + c.x_off, c.Co + 8 + c.ldo_pad, 4 + c.out_off


# ---- E: r3d_gemm_tn ---------------------------------------------------------------------------------------------------
TN = namedtuple("TN", "name M Ca Cb plan rows chunks what")  # plan: bit 0 bf16 x 3, bit 1 256 x 64 tiles (arithmetic 1)
TN_M = (1, 70, 127, 128, 129, 159, 160, 161)
TN_LAST = {129: 1, 159: 31, 160: 32, 161: 33}  # M -> rows of the last 128-row chunk


def _tn():
    out = []
    for m in TN_M:
        ch = -(-m // 128)
        out.append(TN("tn22 M=%d" % m, m, 33, 65, 1, 128, ch, "128 x 128 tiles; last chunk of %d rows" % (m - 128 * (ch - 1))))
        out.append(TN("tn41 M=%d" % m, m, 257, 33, 3, 128, ch, "256 x 64 tiles; last chunk of %d rows" % (m - 128 * (ch - 1))))
    out += [TN("tn22 Ca=%d" % a, 161, a, 65, 1, 128, 2, "Ca on both sides of the 32-row MFMA tile and the 128-row tile; Cb = 65")
            for a in (32, 127, 128, 129, 192)]
    out += [TN("tn22 Cb=%d" % b, 161, 33, b, 1, 128, 2, "Cb one beyond 64 (the smallest 128 x 128 case) .. beyond 128; Ca = 33")
            for b in (128, 129, 192)]
    out += [TN("tn41 Ca=%d" % a, 161, a, 33, 3, 128, 2, "Ca on both sides of the 256-row tile; Cb = 33") for a in (32, 255, 256)]
    out += [TN("tn41 Cb=%d" % b, 161, 257, b, 3, 128, 2, "Cb on both sides of the 32-column MFMA tile, a full 64; Ca = 257")
            for b in (32, 63, 64)]
    out += [TN("tn fp32 Ca=31", 161, 31, 64, 0, 128, 2, "Ca < 32: the fp32 kernel under either arithmetic"),
            TN("tn fp32 Cb=31", 161, 64, 31, 0, 128, 2, "Cb < 32"),
            TN("tn fp32 Cb=9", 161, 128, 9, 0, 128, 2, "the input layer's weight gradient"),
            TN("tn22 65x65", 129, 65, 65, 1, 128, 2, "one beyond the 64 x 64 tile of the fp32 kernel, which arithmetic 0 runs here")]
    return out


TN_CASES = _tn()
TN_EPILOGUE = ("tn22 M=161", "tn41 M=161", "tn fp32 Cb=9")  # crossed with alpha and accumulate
TN_ALPHAS = (1.0, -0.5, 1.0 / 3.0)
