"""The row kernels against float64 references, every element (tests/exact_rows.py): LayerNorm forward and
backward, softmax, cross-entropy and the embedding, through the raw ops, one stage at a time.

Where the result is exactly computable (integer gradients, one rounding of an exact fp32 sum) the comparison is
bitwise; elsewhere each element is held to a bound derived in the case's docstring.  Each case names the
template instantiation and the branch its shape reaches.  The CPU tier, tests/test_exact_rows.py, runs the same
cases on an emulation and shows that each check catches a slip the whole-tensor norm lets through.

What these tests do not hold: the e4m3 / e5m2 bytes of the q8 instantiations (tests/test_fp8_ln_q8_gpu.py holds them
bitwise to the quantisers, which tests/test_fp8_exact_gpu.py holds to the OCP formats); rn_colred1_k / rn_colred2_k, which need more than 4096 column blocks and more than 1024
partial rows at once (docs/DESIGN.md §7).  The ticket kernel rn_colsum_k is reached by
tests/test_gemm_exact_gpu.py::test_act_bwd_bias_grad_ticket_reduction."""

import exact_rows as R
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_problems():
    yield
    R.clear_caches()
    torch.cuda.empty_cache()


# ---- 1. LayerNorm forward -----------------------------------------------------------------------
@pytest.mark.parametrize("residual,bias", R.LN_FORMS)
@pytest.mark.parametrize("E", R.LN_FWD_E)
def test_layernorm_fwd_widths(cuda, E, residual, bias):
    """M = 9: one row per wave, a ragged last block.  E -> NV: 8, 64, 96, 512 -> 1; 520 -> 2 (second chunk: one
    lane); 1032 -> 4 (3 rounded up); 2056 -> 8 (5 rounded up); 4096 -> 8 (full); 4104, 8192 -> 16."""
    R.case_ln_fwd(cuda, 9, E, residual, bias)


@pytest.mark.parametrize("residual,bias", R.LN_FORMS)
@pytest.mark.parametrize("M", R.LN_FWD_M)
def test_layernorm_fwd_rows(cuda, M, residual, bias):
    """E = 64.  M = 1, 4, 5: fewer rows than a block's waves, one block, a ragged second block.  M = 8197 and
    16389: the grid is capped at 8192 waves, so some waves walk 2 or 3 rows and the last prefetch must stay
    inside M."""
    R.case_ln_fwd(cuda, M, 64, residual, bias)


def test_layernorm_fwd_offset_rows(cuda):
    """Rows of mean ~ 64 and spread ~ 1: the saved rstd is right only with the centred two-pass variance."""
    R.case_ln_fwd(cuda, 9, 520, False, True, kind="offset")
    R.case_ln_fwd(cuda, 8197, 64, False, False, kind="offset")


@pytest.mark.parametrize("M,E", [(9, 520), (8197, 64)])
def test_layernorm_fwd_view_of_larger_buffer(cuda, M, E):
    """x is rows 3 .. 3 + M of a sentinel-filled buffer: nothing around (or under) it may change."""
    R.case_ln_fwd(cuda, M, E, True, True, view=True)
    R.case_ln_fwd(cuda, M, E, False, False, view=True)


@pytest.mark.parametrize("E,forms", [(520, R.LN_FORMS), (4104, [(True, True)])])
def test_layernorm_fwd_q8_same_bf16_outputs(cuda, E, forms):
    """ln_fwd_k<2, .., Q8> and <16, .., Q8> at M = 16389 > 4·4096 rows: two rows on some waves of its larger grid."""
    for residual, bias in forms:
        R.case_ln_fwd_q8(cuda, 16389, E, residual, bias)


# ---- 2. LayerNorm backward ----------------------------------------------------------------------
@pytest.mark.parametrize("gh,dxs", R.LN_FORMS)
@pytest.mark.parametrize("E", R.LN_BWD_FORMS_E)
def test_layernorm_bwd_forms(cuda, E, gh, dxs):
    """The four ln_bwd_k<NV, GH, DXS> forms at NV = 1, 2, 16; M = 2051: 512 blocks, three waves walk two rows."""
    R.case_ln_bwd(cuda, 2051, E, gh, dxs)


@pytest.mark.parametrize("E", R.LN_BWD_E)
def test_layernorm_bwd_widths(cuda, E):
    """M = 9, plain.  NV = 1 (8, 512), 4 (1032), 8 (2056, 4096) and the full NV = 16 at E = 8192: ln_bwd_k<16>
    with its 96 KiB of LDS, which no test ran before."""
    R.case_ln_bwd(cuda, 9, E, False, False)


@pytest.mark.parametrize("M", R.LN_BWD_M)
def test_layernorm_bwd_rows(cuda, M):
    """E = 64.  M = 1, 5: a single partial row; 2051, 4099: 512 partial rows, 2 and 3 rows on some waves."""
    R.case_ln_bwd(cuda, M, 64, False, False)


@pytest.mark.parametrize("M,E", [(2051, 96), (4099, 64)])
def test_layernorm_bwd_accumulate(cuda, M, E):
    """dw_accum / db_accum: the column kernel adds into integer-valued bf16 gradients; db bitwise."""
    R.case_ln_bwd(cuda, M, E, True, True, accumulate=True)


# ---- 4. softmax and cross-entropy ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused", "two_pass"])
@pytest.mark.parametrize("V", list(R.XENT_V))
def test_cross_entropy_rows(cuda, V, mode):
    """exact_rows.XENT_V says which kernel and branch V reaches; n_valid = V, V - 3 (a straddling chunk) and
    V - 47 (whole padded chunks and a straddling one); 8, 5, 1 at V = 8."""
    for nvalid in R.xent_nvalids(V):
        R.case_xent(cuda, V, nvalid, mode)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("N", R.SOFTMAX_N)
def test_softmax_rows(cuda, N, scale):
    """row_ms: the vector loop on 16-byte aligned rows, the scalar one on the others (N = 7, 197, 2049: every row
    but the first) and for the tail N % 8; N = 2049: two vector passes per thread."""
    R.case_softmax(cuda, N, scale)


# ---- 5. embedding -------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [False, True])
@pytest.mark.parametrize("E", [8, 64, 520, 768])
def test_embedding_fwd(cuda, E, pos):
    """emb_fwd_k<POS>: E = 8 one lane, 520 a second pass of one lane, 768 two passes; rows 1, 5, 123."""
    for shape in [(1,), (5,), (123,), (3, 41)]:
        R.case_embedding_fwd(cuda, E, shape, pos)


@pytest.mark.parametrize("E", [8, 64, 768])
def test_embedding_bwd_scatter(cuda, E):
    """emb_bwd_scatter_k (fp32 atomics into a zeroed table), f32_to_bf16_k, emb_bwd_pos_k with Tp > T."""
    R.case_embedding_bwd(cuda, E)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("E", [8, 64, 260, 768])
def test_embedding_bwd_accumulate_three_calls(cuda, E, deterministic, monkeypatch):
    """emb_scatter_own_k / emb_finish_k, or their 2^40 fixed-point forms under REPLICANN_DETERMINISTIC=1, and
    emb_pos_acc_k; E = 260: E % 4 only (the float4 finish with a ragged last pass)."""
    R.case_embedding_bwd_acc(cuda, E, setenv=monkeypatch.setenv, deterministic=deterministic)
