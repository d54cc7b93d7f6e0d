"""The fp8 quantisers of csrc/kernels/fp8.hip against the OCP formats, every byte and every state slot
(tests/exact_fp8.py), through the raw ops.

Bitwise: fp8_quantize, fp8_quantize_delayed, bf8_quantize (both modes), fp8_quant_many, both dequantisers,
act_mul_bf8(from_h=False) with its bias gradient on grid-valued inputs.  Within a derived bound, with at most 1 % of the
elements allowed a second accepted byte: gelu_q8, act_mul_bf8(from_h=True), and act_mul_bf8's bias gradient on table
inputs.  Each test names the branch its shape reaches; the shapes are the smallest that reach it.  The CPU tier,
tests/test_exact_fp8.py, checks the references against each other and shows that every check fails on a quantiser
that is wrong in one way.

Not held here: non-finite inputs, n = 0, and value tables fed through the fused producers (LayerNorm q8, the
GEMM epilogue, the attention backward), which stay anchored by their bitwise comparison with the ops tested here
(tests/test_fp8_ln_q8_gpu.py, tests/test_ops_gpu.py)."""

import exact_fp8 as X
import pytest
import torch

pytestmark = pytest.mark.gpu

FMTS = [X.E4M3, X.E5M2]
fmt_ids = lambda f: f.name  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _drop_tables():
    yield
    X.clear_caches()
    torch.cuda.empty_cache()


# ---- 1. current scaling -------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(X.SIZES))
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_ids)
def test_current_scaling(cuda, fmt, n):
    """amax_k + quant_k (e4m3) / quant_bf8_k (e5m2).  n: exact_fp8.SIZES names the branch.  For k in {-20, 0, 10} the
    planted amax is exactly max · 2^k, one bf16 ulp above (the scale doubles) and one below; it sits at element 0, only
    in the scalar tail, or only in the second grid-stride trip, wherever n has such an element."""
    ran = 0
    for k in X.KS:
        for cls in X.AMAX_CLASSES:
            for plant in X.PLANTS:
                ran += X.case_current(cuda, fmt, n, k, cls, plant)
    assert ran == 9 * (1 + (n % 8 != 0 and n > 8) + (n == X.N_BIG))


@pytest.mark.parametrize("fmt", FMTS, ids=fmt_ids)
def test_current_scaling_tiny_tensor(cuda, fmt):
    """amax = 2^-120: the subnormal quotient amax / max must give the smallest normal scale, not pow2_ceil(0) = 1."""
    assert X.case_tiny(cuda, fmt) == 2.0**-126


# ---- 2. delayed scaling -------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(X.SIZES) + [X.N_UNROLL])
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_ids)
def test_delayed_scaling_two_calls(cuda, fmt, n):
    """fp8_roll_k + quant_delayed_k / fp8_roll_bf8_k + quant_delayed_bf8_k, two calls on one state, from a previous amax
    of 0, one that makes the table saturate and one that makes most of it underflow.  n = 8·(3·524288 + 1000) + 5 is
    the smallest at which quant_delayed_bf8_k's 4-chunk loop runs (threads below 1000 once; all others take the
    remainder loop three times; then the tail); the e4m3 kernel gets the same size."""
    for prev in X.PREVS:
        X.case_delayed(cuda, fmt, n, prev)


@pytest.mark.parametrize("n", [2053, X.N_BIG, X.N_UNROLL])
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_ids)
def test_position_pattern(cuda, fmt, n):
    """The expected bytes are the index pattern: a swap inside a chunk or a chunk in another's place is a shifted index."""
    X.case_position(cuda, fmt, n, True)
    if n != X.N_UNROLL:
        X.case_position(cuda, fmt, n, False)


# ---- 3. the weight cache's quantiser --------------------------------------------------------------
@pytest.mark.parametrize("roll", [True, False])
def test_quant_many(cuda, roll):
    """fp8_roll_many_k + fp8_quant_many_k on a hand-built buffer: segments of 5, 1000, 2400 and 300 003 elements, the
    last three sweeps of the 64-block cap; the padding keeps its sentinel; bytes and state equal the single-tensor op."""
    X.case_quant_many(cuda, roll)


# ---- 4. dequantise ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", X.DEQ_N)
@pytest.mark.parametrize("fmt", FMTS, ids=fmt_ids)
def test_dequantise_every_code(cuda, fmt, n):
    """dequant_k / dequant_bf8_k on all 256 codes; scales 2^-20, 1, 2^10 and 0.3 (a rounded fp32 product)."""
    for scale in X.DEQ_SCALES:
        X.case_dequant(cuda, fmt, n, scale)


# ---- 5. act_mul_bf8, from_h = False ---------------------------------------------------------------
@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("M,N", X.ACT_MUL_SMALL)
def test_act_mul_small(cuda, M, N, delayed):
    """act_mul_bf8_k<0> + <1> (current) / <2> (delayed).  (1, 8): one live thread; (7, 24): 21 live threads, dead ones
    inside block_max; (5, 1000): G = M, 625 threads, a ragged third block."""
    for k in X.KS:
        X.case_act_mul(cuda, M, N, k, delayed)
    X.case_act_mul_bias_grid(cuda, M, N, delayed)
    X.case_act_mul_bias_table(cuda, M, N)


@pytest.mark.parametrize("delayed", [False, True])
def test_act_mul_four_row_loop(cuda, delayed):
    """(5·2048 + 3, 1024): G = 2048, so every thread runs the 4-row loop once and the remainder loop once (twice for
    the first three row groups); the bias gradient goes through the ticketed rn_colsum_k (2048 partial rows)."""
    M, N = X.ACT_MUL_LARGE
    assert X.act_mul_groups(M, N) == 2048
    X.case_act_mul(cuda, M, N, -20, delayed)
    X.case_act_mul_bias_grid(cuda, M, N, delayed)
    if not delayed:
        X.case_act_mul_bias_table(cuda, M, N)


# ---- 6. the GELU producers: bounded -----------------------------------------------------------------
@pytest.mark.parametrize("n", X.GELU_N)
def test_gelu_q8(cuda, n):
    """gelu_q8_k on every finite bf16 |h| <= 16; n = 8·(8192·256 + 300) is a second trip of its 8192-block grid."""
    X.case_gelu_q8(cuda, n)


@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("M,N", X.FROM_H)
def test_act_mul_from_h(cuda, M, N, delayed):
    """act_mul_bf8_k<.., true>: gelu'(h) taken in the kernel; (4099, 64): G = 4099, one row per thread, 129 blocks."""
    X.case_act_mul_from_h(cuda, M, N, delayed)
