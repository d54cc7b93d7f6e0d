"""The HIP GEMMs against exact expected outputs, every element, every tile config (tests/exact_ints.py).

With small integer operands every product and every fp32 partial sum is exact, so the output of a correct
kernel is the one bf16 rounding of the float64 product: bit for bit, whatever the tile shape, accumulation
order, split-K or wait count.  A wrong ragged-tail fragment, a tile finished one K-tile early, a dropped
split-K slab or an unreduced column-partial row changes elements, and assert_bitwise names them.  The
references are float64 matmuls on the GPU, computed once per problem and shared by its configs.

Groups: a plain products (all four layouts; N, K, M not multiples of 8; out views); b exact epilogues;
c activation backward with the fused bias gradient; d GELU epilogues, the one place with a bound (per
element, derived at exact_ints.gelu_report); e fp8; f convolution as GEMM.

fp8: the scaled f8f6f4 MFMA sums of in-range integers met bitwise equality on the MI355X (all three
REPLICANN_FP8_GEMM kernels plain and with bias, the data gradient from e5m2 and from e4m3, the weight
gradient into bf16 / fp32 / accumulated fp32), so the cases assert it; the one-ulp form was not needed.

The residual: the epilogue staged through LDS keeps act(h + bias) as a bf16 tile and adds the residual to
that stored value (two roundings); the direct epilogue, the split-K reduce and cfg 9 / 11 without an
activation add it in fp32 (one).  Both values are exactly computable, so each config is held, bit for bit
and in every element, to the form its epilogue is documented to give (docs/DESIGN.md): see
exact_ints.case_residual.  Measured on the MI355X, the two forms differ in 342 of 14400 (200x72x96), 30023 of
403520 (520x776x1088) and 612668 of 16859200 (8200x2056x128) elements with bias + residual.
"""

import exact_ints as E
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_problems():
    yield
    E.clear_caches()
    torch.cuda.empty_cache()


# ---- a: the plain product -----------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", E.LAYOUTS)
@pytest.mark.parametrize("M,N,K", E.RAGGED + E.ODD + E.PERSISTENT)
def test_plain_every_config(cuda, M, N, K, ta, tb):
    cfgs = E.TILE_CFGS + ((11,) if E.w1_takes(M, N, K, ta, tb) else ())
    views = ()
    if (M, N, K) in ((520, 776, 1088), (8200, 2056, 128)) and not ta:
        views = (1, 9, 11)  # into a view of a sentinel-filled buffer: nothing outside it is written
    E.case_plain(cuda, M, N, K, ta, tb, cfgs=cfgs, view_cfgs=views)


@pytest.mark.parametrize("M,N,K", E.SKINNY)
def test_skinny_decode_gemm(cuda, M, N, K):
    E.case_skinny(cuda, M, N, K)


# ---- b: epilogues that stay exact ---------------------------------------------------------------
EPILOGUE_SHAPES = [(200, 72, 96), (520, 776, 1088), (8200, 2056, 128)]
STAGED_CFGS = (0, 1, 2, 3, 4, 5, 6, 8)  # gemm_impl.h: the epilogue staged through LDS as bf16


@pytest.mark.parametrize("M,N,K", EPILOGUE_SHAPES)
def test_exact_epilogues(cuda, M, N, K):
    E.case_epilogues(cuda, M, N, K, with_w1=True)


def _residual_params():
    """(shape, cfg, relu, form).  Staged configs round twice; cfg 9 once, but twice when it also saves a
    pre-activation; cfg 11 (17 K-tiles: its residual bodies) once; cfg -1 runs one of these, picked by time."""
    out = []
    for M, N, K in EPILOGUE_SHAPES:
        for relu in (False, True):
            w1 = (11,) if not relu and (M, N, K) == (520, 776, 1088) else ()
            for cfg in STAGED_CFGS + (9, -1) + w1:
                rounds = "either" if cfg == -1 else "twice" if cfg in STAGED_CFGS or relu else "once"
                out.append(pytest.param(M, N, K, cfg, relu, rounds,
                                        id=f"{M}-{N}-{K}-cfg{cfg}-{'relu' if relu else 'plain'}-{rounds}"))
    return out


@pytest.mark.parametrize("M,N,K,cfg,relu,rounds", _residual_params())
def test_residual_every_element(cuda, M, N, K, cfg, relu, rounds):
    if cfg == 11:
        assert E.w1_takes(M, N, K, False, True) and K // 64 >= 6
    E.case_residual(cuda, M, N, K, cfg, relu, rounds)


@pytest.mark.parametrize("M,N,K", [(200, 72, 96), (520, 776, 1088)])
def test_explicit_split_k(cuda, M, N, K):
    E.case_split_k(cuda, M, N, K)


@pytest.mark.parametrize("M,N,K", [(200, 72, 96), (520, 776, 1088)])
def test_accumulate_bf16(cuda, M, N, K):
    E.case_accumulate_bf16(cuda, M, N, K)


# ---- c: activation backward with the fused bias gradient ----------------------------------------
@pytest.mark.parametrize("act", [3, 6])
@pytest.mark.parametrize("M,N,K", E.ACT_BWD)
def test_act_bwd_bias_grad(cuda, M, N, K, act):
    E.case_act_bwd(cuda, M, N, K, act)


@pytest.mark.parametrize("M,N,K", E.ACT_BWD)
def test_act_bwd_bias_grad_captured(cuda, M, N, K):
    """cfg = -1 while the stream is captured, on a problem no tuning table holds (no eager call tunes an
    activation-backward problem of these shapes: the eager cases give cfg or split_k): the binding keeps the
    request -1 and has to size the column-partial reduction from the config that runs."""
    a, b, pre, bg0, exp, exp_bg = E.bwd_problem(str(cuda), M, N, K, 6)
    bg = bg0.clone()
    out = torch.empty(M, N, device=cuda, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        E.gemm_bwd(a, b, 6, pre, out=out, bias_grad=bg)
    graph.replay()
    torch.cuda.synchronize()
    E.assert_bitwise(out, exp, what="captured cfg -1: out")
    E.assert_bitwise(bg.view(1, -1), exp_bg.view(1, -1), what="captured cfg -1: bias_grad")


def test_act_bwd_bias_grad_ticket_reduction(cuda):
    """More than 1024 column-partial rows: rn_colreduce_seg leaves the one-block rn_colsum1_k for rn_colsum_k,
    whose blocks hand their slab sums over write-through, take an arrival ticket, and whose last arriver sums the
    slabs and re-arms the counter.  Only the configs that emit column partials; twice in one process: the second
    run passes only if every counter was reset."""
    M, N, K = E.ACT_BWD_TICKET
    assert 2 * ((M + 255) // 256) > 1024 and (M + 127) // 128 > 1024  # gemm_colpart_rows: cfg 9, the 128-row configs
    for _ in range(2):
        E.case_act_bwd(cuda, M, N, K, 3, variants=E.BWD_COLPART, strided=())


def test_bias_grad_unaligned_rows(cuda):
    E.case_bias_grad_unaligned(cuda, 300, 264)


def test_bias_grad_rejects_fp32_out(cuda):
    """Both reductions of the fused bias gradient read bf16 rows; an fp32 output is refused, not misread."""
    a, b, pre, bg0, _, _ = E.bwd_problem(str(cuda), 300, 264, 192, 6)
    out = torch.zeros(300, 264, device=cuda)
    with pytest.raises(RuntimeError, match="bf16 output"):
        E.gemm_bwd(a, b, 6, pre, out=out, bias_grad=bg0.clone())


# ---- d: GELU epilogues --------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,density", E.GELU)
def test_gelu_epilogues(cuda, M, N, K, density):
    E.case_gelu(cuda, M, N, K, density)


@pytest.mark.parametrize("M,N,K,density", E.GELU)
def test_gelu_bwd_epilogue(cuda, M, N, K, density):
    E.case_gelu_bwd(cuda, M, N, K, density)


# ---- e: fp8 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", E.FP8_FWD)
def test_fp8_forward(cuda, M, N, K, monkeypatch):
    E.case_fp8_fwd(cuda, M, N, K, setenv=monkeypatch.setenv)


# REPLICANN_FP8_GEMM=0 and, below K = 2048, =11 stage h + bias as bf16 (two roundings); =9, and =11 on its
# K >= 2048 persistent path, add the residual in fp32 (one)
FP8_RESIDUAL = [((1000, 776, 512), "11", "twice"), ((1000, 776, 512), "9", "once"), ((1000, 776, 512), "0", "twice"),
                ((8200, 2056, 2048), "11", "once"), ((8200, 2056, 2048), "9", "once"),
                ((8200, 2056, 2048), "0", "twice")]


@pytest.mark.parametrize("shape,mode,rounds", FP8_RESIDUAL, ids=[f"{s[0]}-{s[1]}-{s[2]}-mode{m}-{r}" for s, m, r in FP8_RESIDUAL])
def test_fp8_residual_every_element(cuda, shape, mode, rounds, monkeypatch):
    E.case_fp8_residual(cuda, *shape, mode, setenv=monkeypatch.setenv, rounds=rounds)


@pytest.mark.parametrize("a_bf8", [True, False])
@pytest.mark.parametrize("M,N,K", E.FP8_DGRAD)
def test_fp8_dgrad(cuda, M, N, K, a_bf8):
    E.case_fp8_dgrad(cuda, M, N, K, a_bf8)


@pytest.mark.parametrize("M,N,K", E.FP8_WGRAD)
def test_fp8_wgrad(cuda, M, N, K):
    E.case_fp8_wgrad(cuda, M, N, K)


# ---- f: convolution as GEMM ---------------------------------------------------------------------
@pytest.mark.parametrize("C,OC,k,S,P,HW", E.CONV)
def test_conv_as_gemm(cuda, C, OC, k, S, P, HW):
    E.case_conv(cuda, C, OC, k, S, P, HW)
