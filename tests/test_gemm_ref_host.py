"""tests/gemm_ref.py against torch in float64, and the claims of tests/gemm_cases.py against the host functions the launchers
branch on (r3d_debug_pointwise_path, r3d_debug_gemm_tn_plan) -- no GPU.  What tests/test_gpu_gemm_kernels.py measures the
kernels against, and which kernel each of its cases reaches, is settled here."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import gemm_cases as C
import gemm_ref as R


@pytest.fixture(scope="module")
def lib():
    from r3dfsseg_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def setting(lib, arith, mask):
    """r3d_set_matrix_arith(arith) and r3d_debug_set_gemm_bx3(mask) for the block.  The mask has no getter: afterwards it is
    what the process started with (_lib.load: R3D_GEMM_BX3, else all three bits)."""
    from r3dfsseg_amd import _lib
    a0 = lib.r3d_get_matrix_arith()
    _lib.check(lib.r3d_set_matrix_arith(arith))
    _lib.check(lib.r3d_debug_set_gemm_bx3(mask))
    try:
        yield
    finally:
        _lib.check(lib.r3d_debug_set_gemm_bx3(int(os.environ.get("R3D_GEMM_BX3", 7))))
        _lib.check(lib.r3d_set_matrix_arith(a0))


def tn_plan(lib, M, Ca, Cb):
    rows, chunks = ctypes.c_int(-1), ctypes.c_int(-1)
    plan = lib.r3d_debug_gemm_tn_plan(M, Ca, Cb, ctypes.byref(rows), ctypes.byref(chunks))
    return plan, rows.value, chunks.value


def _rand(shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32))


@pytest.mark.parametrize("act", C.ACTS)
@pytest.mark.parametrize("given", C.AFFINE)
@pytest.mark.parametrize("acc", [0, 1])
def test_pointwise_restatement_is_torch_in_float64(act, given, acc):
    M, K, Co = 37, 21, 13
    X, W, pre = _rand((M, K), 1), _rand((Co, K), 2), _rand((M, Co), 5)
    sc = _rand((Co,), 3) if given[0] else None
    sh = _rand((Co,), 4) if given[1] else None
    z = torch.nn.functional.linear(X.double(), W.double())
    if sc is not None:
        z = z * sc.double()
    if sh is not None:
        z = z + sh.double()
    z = (z, torch.relu(z), torch.nn.functional.leaky_relu(z, 0.2))[act]
    want = (pre.double() + z) if acc else z
    got = R.pointwise(X, W, sc, sh, act, pre if acc else None)
    assert got.dtype == np.float64
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-13, atol=1e-13)
    g32 = R.pointwise32(X, W, sc, sh, act, pre if acc else None)
    bound = R.pointwise_bound(X, W, sc, sh, pre if acc else None)
    assert g32.dtype == np.float32 and 0 < R.figure(g32, got, bound) < K * 2.0 ** -24  # fp32 it is, and no worse than K ulps
    # the bound: |scale| sum |x||w| + |shift| (+ |pre|), element by element
    b = X.double().abs() @ W.double().abs().t()
    b = b * (sc.double().abs() if given[0] else 1.0) + (sh.double().abs() if given[1] else 0.0) + (pre.double().abs() if acc else 0.0)
    np.testing.assert_allclose(bound, b.numpy(), rtol=1e-13)


@pytest.mark.parametrize("alpha", C.TN_ALPHAS)
@pytest.mark.parametrize("acc", [0, 1])
def test_gemm_tn_restatement_is_torch_in_float64(alpha, acc):
    M, Ca, Cb = 45, 11, 7
    A, B, pre = _rand((M, Ca), 6), _rand((M, Cb), 7), _rand((Ca, Cb), 8)
    a32 = float(np.float32(alpha))
    want = a32 * (A.double().t() @ B.double()) + (pre.double() if acc else 0.0)
    got = R.gemm_tn(A, B, alpha, pre if acc else None)
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-13, atol=1e-13)
    g32 = R.gemm_tn32(A, B, alpha, pre if acc else None)
    bound = R.gemm_tn_bound(A, B, alpha, pre if acc else None)
    assert g32.dtype == np.float32 and 0 < R.figure(g32, got, bound) < M * 2.0 ** -24
    b = abs(a32) * (A.double().abs().t() @ B.double().abs()) + (pre.double().abs() if acc else 0.0)
    np.testing.assert_allclose(bound, b.numpy(), rtol=1e-13)


def test_figure_demands_exact_zeros_where_nothing_was_summed():
    ref, bound = np.array([[0.0, 2.0]]), np.array([[0.0, 4.0]])
    assert R.figure(np.array([[-0.0, 3.0]], np.float32), ref, bound) == 0.25
    with pytest.raises(AssertionError):
        R.figure(np.array([[1e-30, 2.0]], np.float32), ref, bound)
    with pytest.raises(AssertionError):
        R.figure(np.array([[0.0, np.nan]], np.float32), ref, bound)


def test_every_pointwise_case_reaches_the_path_it_claims(lib):
    cases = C.SWEEPS + C.EPILOGUE + [C.GROW_SMALL, C.GROW_LARGE]
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        ldx, _, ldo, _ = C.pw_geometry(c)  # the slices of the GPU module: column 4 of an aligned wide matrix
        with setting(lib, 1, c.mask):
            assert lib.r3d_debug_pointwise_path(c.M, c.K, c.Co, ldx, ldo, 0, 0, 0, 0) == c.path, c
            assert lib.r3d_debug_pointwise_path(c.M, c.K, c.Co, ldx, ldo, 0, 0, 0, 1) == min(c.path, 1), c  # no scratch: 2 -> 1
        with setting(lib, 0, c.mask):
            assert lib.r3d_debug_pointwise_path(c.M, c.K, c.Co, ldx, ldo, 0, 0, 0, 0) == 0, c
        assert c.M <= 1024


def test_the_pointwise_tables_claim_every_path_edge_and_variant():
    by = {p: [c for c in C.SWEEPS if c.path == p and c.mask == 7] for p in (0, 1, 2)}
    m3 = [c for c in C.SWEEPS if c.mask == 3]
    assert {c.M for c in by[0]} >= set(C.FP32_M) == {1, 63, 64, 65, 129}
    assert {c.Co for c in by[0]} >= set(C.FP32_CO) == {1, 31, 63, 64, 65}
    assert {c.K for c in by[0]} >= set(C.FP32_K) == {1, 9, 31, 32, 33, 64, 65, 100}
    assert {c.M for c in by[1]} >= {64, 65, 127, 128, 129, 255} and {c.M for c in m3} == {256, 257, 511, 513}
    assert all(c.path == 1 for c in m3)
    assert {c.M for c in by[2]} >= {256, 257, 281, 287, 288, 289, 383, 384, 385}
    for p in (1, 2):
        assert {c.Co for c in by[p]} >= {32, 36, 60, 64, 68, 96, 128, 132, 160, 192}
        assert {c.K for c in by[p]} >= {32, 64, 96, 160}
    # B: a full-tile and a tail shape per kernel; the packed kernel's six variants, each with accumulate where the ABI
    # reaches it (r3d_pointwise_conv_acc: no statistics; r3d_pointwise_conv_stats: no accumulate)
    assert sorted(c.path for c in C.EPILOGUE) == [0, 0, 1, 1, 2, 2]
    seen = set()
    for c in C.EPILOGUE:
        if c.path == 2:
            seen |= C.packed_variants(c.M, c.Co, plain=True, stats=True)     # r3d_pointwise_conv_stats
            seen |= C.packed_variants(c.M, c.Co, plain=True, stats=False)    # (NULL, NULL), act 0; also with accumulate
            seen |= C.packed_variants(c.M, c.Co, plain=False, stats=False)   # every other row of the cross; also with accumulate
    assert seen == C.PACKED_VARIANTS and len(seen) == 6
    full, tail = (c for c in C.EPILOGUE if c.path == 2)
    assert {v[2] for v in C.packed_variants(full.M, full.Co, True, False)} == {True}
    assert {v[2] for v in C.packed_variants(tail.M, tail.Co, True, False)} == {True, False}
    assert C.packed_variants(257, 132, False, True) == {(False, True, False)}
    assert (0, 0) in C.AFFINE and len(set(C.AFFINE)) == 4 and C.ACTS == (0, 1, 2)


def test_every_fallback_rule_sends_the_base_shape_to_the_fp32_kernel(lib):
    """(256, 64, 64) takes the packed kernel; each case breaks one rule and r3d_debug_pointwise_path says 0 -- the ldo and
    Out rules included, which r3d_pointwise_bx3_launch used to decide after r3d_pointwise_bx3_ok had said yes."""
    assert {c.rule for c in C.FALLBACKS} >= set(C.FALLBACK_RULES) and len(C.FALLBACK_RULES) == 9
    with setting(lib, 1, 7):
        assert lib.r3d_debug_pointwise_path(256, 64, 64, 72, 72, 0, 0, 0, 0) == 2
        for c in C.FALLBACKS:
            ldx, x0, ldo, o0 = C.fb_geometry(c)
            assert ldx >= x0 + c.K and ldo >= o0 + c.Co
            args = (c.M, c.K, c.Co, ldx, ldo, 4 * x0 % 16, 4 * c.w_off % 16, 4 * o0 % 16)
            assert lib.r3d_debug_pointwise_path(*args, 0) == 0 and lib.r3d_debug_pointwise_path(*args, 1) == 0, c
            # exactly one rule is broken: mending it gives a bf16 path
            rules = [c.K % 32 != 0 or c.K < 32, c.Co < 32, c.Co % 4 != 0, c.M < 64, ldx % 4 != 0, x0 % 4 != 0, c.w_off % 4 != 0,
                     o0 % 4 != 0, ldo % 4 != 0]
            assert sum(rules) == 1, (c, rules)


def test_tn_plan_of_every_case(lib):
    assert len({c.name for c in C.TN_CASES}) == len(C.TN_CASES)
    for c in C.TN_CASES:
        with setting(lib, 1, 7):
            assert tn_plan(lib, c.M, c.Ca, c.Cb) == (c.plan, c.rows, c.chunks), c
        with setting(lib, 1, 5):  # bit 1 of the mask off: the weight-gradient GEMM stays on the fp32 core
            assert tn_plan(lib, c.M, c.Ca, c.Cb) == (0, c.rows, c.chunks), c
        with setting(lib, 0, 7):
            assert tn_plan(lib, c.M, c.Ca, c.Cb) == (0, c.rows, c.chunks), c
        assert lib.r3d_gemm_tn_ws_words(c.M, c.Ca, c.Cb) == c.chunks * c.Ca * c.Cb + 16
    for m, last in C.TN_LAST.items():  # chunks of 128 rows: the last one has 1, 31, 32, 33
        assert m - 128 == last and any(c.M == m and c.rows == 128 and c.chunks == 2 for c in C.TN_CASES)
    assert sorted(C.TN_LAST.values()) == [1, 31, 32, 33] and set(C.TN_M) >= {1, 70, 127, 128}
    t22 = [c for c in C.TN_CASES if c.plan == 1]
    t41 = [c for c in C.TN_CASES if c.plan == 3]
    f32 = [c for c in C.TN_CASES if c.plan == 0]
    assert all(c.Cb > 64 for c in t22) and all(c.Cb <= 64 for c in t41) and all(min(c.Ca, c.Cb) < 32 for c in f32)
    assert {c.Ca for c in t22} >= {32, 33, 127, 128, 129, 192} and {c.Cb for c in t22} >= {65, 128, 129, 192}
    assert {c.Ca for c in t41} >= {32, 255, 256, 257} and {c.Cb for c in t41} >= {32, 33, 63, 64}
    assert any(c.Cb == 9 for c in f32) and any(c.Ca < 32 for c in f32)
    assert {c.name for c in C.TN_CASES} >= set(C.TN_EPILOGUE)
    assert {c.plan for c in C.TN_CASES if c.name in C.TN_EPILOGUE} == {0, 1, 3}
    # a long M axis: more chunks than one, of more rows than 128 (the plan the model's weight gradients take)
    with setting(lib, 1, 7):
        assert tn_plan(lib, 786432, 512, 192) == (1, 4096, 192)
