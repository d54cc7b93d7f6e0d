"""CPU tier of the exact GEMM checks (tests/exact_ints.py): every case of tests/test_gemm_exact_gpu.py on CPU
tensors, where ``ops.gemm`` is fp32 ATen math and exact on integer operands.  This validates each generator,
each precondition (asserted inside the cases) and each expected-value formula on a machine with no GPU.

Why the exact tests exist: the norm metric of the other GEMM tests, ||out - ref|| / ||ref|| over the whole
tensor, cannot see a localised error (test_one_ulp_at_the_ragged_corner)."""

import exact_ints as E
import pytest
import torch

CPU = torch.device("cpu")


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_problems():
    yield
    E.clear_caches()


def test_one_ulp_at_the_ragged_corner():
    """One element of a 4352x4200 output, one bf16 ulp off, in the last ragged tile: the whole-tensor norm
    of test_gemm_persistent_multi_tile passes it, assert_bitwise fails and names the tile."""
    M, N = 4352, 4200
    exp = (torch.randn(M, N, generator=E.gen(0)) * 16).to(torch.bfloat16)
    out = exp.clone()
    r, c = M - 1, N - 1
    out.view(torch.int16)[r, c] += 1
    rel = ((out.float() - exp.float()).norm() / exp.float().norm()).item()
    assert rel < 1e-2  # the old bound: blind
    E.assert_bitwise(exp.clone(), exp)
    with pytest.raises(AssertionError) as ei:
        E.assert_bitwise(out, exp)
    msg = str(ei.value)
    assert "1 of %d elements differ" % (M * N) in msg
    assert f"first at ({r}, {c})" in msg
    assert f"[({r // 256}, {c // 256})]" in msg  # tile (16, 16), the ragged corner
    assert f"rows {r // 16 * 16}.., cols {c // 16 * 16}.." in msg


def test_assert_bitwise_fp32_and_signed_zero():
    a = torch.tensor([[0.0, 1.0, 3.0]])
    z = torch.tensor([[-0.0, 1.0, 3.0]])
    with pytest.raises(AssertionError):  # the raw bits: -0 is not +0 ...
        E.assert_bitwise(z, a)
    E.assert_bitwise(z, a, zero_sign=False)  # ... unless a case says so (activation backward)
    b = a.clone()
    b.view(torch.int32)[0, 2] += 1
    with pytest.raises(AssertionError):
        E.assert_bitwise(b, a)
    with pytest.raises(AssertionError):  # never a comparison across dtypes
        E.assert_bitwise(a.bfloat16(), a)


def test_int_operand_and_rounding_range():
    g = E.gen(1)
    v = E.int_operand((64, 64), -4, 4, density=0.5, generator=g)
    assert v.dtype == torch.bfloat16 and float(v.abs().max()) <= 4 and bool((v == v.round()).all())
    assert 0.4 < float((v == 0).float().mean()) < 0.7  # half thinned, a ninth drawn as 0
    assert [E.rounding_hi(K) for K in (8, 72, 128, 384, 2048)] == [12, 7, 6, 4, 4]
    with pytest.raises(AssertionError):
        E.require_rounding(torch.ones(8, 8, dtype=torch.float64))  # nothing rounds
    with pytest.raises(AssertionError):
        E.require_representable(torch.full((2, 2), 257.0))


@pytest.mark.parametrize("ta,tb", E.LAYOUTS)
@pytest.mark.parametrize("M,N,K", E.RAGGED + E.ODD + E.PERSISTENT)
def test_plain(M, N, K, ta, tb):
    E.case_plain(CPU, M, N, K, ta, tb, cfgs=(-1,), view_cfgs=(-1,))


@pytest.mark.parametrize("M,N,K", E.SKINNY)
def test_skinny(M, N, K):
    E.case_skinny(CPU, M, N, K, splits=(0,))


@pytest.mark.parametrize("M,N,K", [(200, 72, 96), (520, 776, 1088), (8200, 2056, 128)])
def test_epilogues(M, N, K):
    E.case_epilogues(CPU, M, N, K, cfgs=(-1,))
    E.case_residual(CPU, M, N, K, -1, relu=False)
    E.case_residual(CPU, M, N, K, -1, relu=True)
    E.case_split_k(CPU, M, N, K, cfgs=(-1,), splits=(2,))
    E.case_accumulate_bf16(CPU, M, N, K, cfgs=(-1,))


@pytest.mark.parametrize("act", [3, 6])
@pytest.mark.parametrize("M,N,K", E.ACT_BWD)
def test_act_bwd(M, N, K, act):
    E.case_act_bwd(CPU, M, N, K, act, variants=((-1, 0),), strided=((-1, 0, 16), (-1, 0, 4)))


def test_act_bwd_ticket_shape():
    E.case_act_bwd(CPU, *E.ACT_BWD_TICKET, 3, variants=((-1, 0),), strided=())


def test_bias_grad_unaligned():
    E.case_bias_grad_unaligned(CPU, 300, 264)


@pytest.mark.parametrize("M,N,K,density", E.GELU)
def test_gelu(M, N, K, density):
    E.case_gelu(CPU, M, N, K, density, cfgs=(-1,))
    E.case_gelu_bwd(CPU, M, N, K, density, cfgs=(-1,))


@pytest.mark.parametrize("M,N,K", E.FP8_FWD)
def test_fp8_fwd(M, N, K):
    E.case_fp8_fwd(CPU, M, N, K, modes=("cpu",))
    E.case_fp8_residual(CPU, M, N, K, "cpu")


@pytest.mark.parametrize("a_bf8", [True, False])
@pytest.mark.parametrize("M,N,K", E.FP8_DGRAD)
def test_fp8_dgrad(M, N, K, a_bf8):
    E.case_fp8_dgrad(CPU, M, N, K, a_bf8)


@pytest.mark.parametrize("M,N,K", E.FP8_WGRAD)
def test_fp8_wgrad(M, N, K):
    E.case_fp8_wgrad(CPU, M, N, K)


@pytest.mark.parametrize("C,OC,k,S,P,HW", E.CONV)
def test_conv(C, OC, k, S, P, HW):
    E.case_conv(CPU, C, OC, k, S, P, HW)
