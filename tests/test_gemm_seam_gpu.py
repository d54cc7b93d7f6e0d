"""The persistent GEMM's epilogue (cfg 9, csrc/include/gemm_pk.h) on exact integer operands, at the tile seams.

The epilogue form of a launch (bias, residual, accumulate, alpha, ...) picks a kernel instance
(pk_launch_layout); the instance addresses a tile by one per-lane offset per column half plus wave-uniform
row steps, with the M tail in the buffer descriptor's size.  The shapes are the smallest at which that can go
wrong: M of 1, 255, 257, 385 (one and two 256-row tiles, a ragged last 16-row fragment, a ragged half), N of
8, 40 (the ragged bias block), 264, 392 (tail in the left / right column half), K of 64 (one K-tile) and 320
(the shortest item of the dynamic schedule: static and dynamic).  Every element of every output is compared
bit for bit with the one rounding of the exact float64 value (tests/exact_ints.py); only the GELU outputs
have a bound, exact_ints.gelu_report's.

Forms with an instance of their own: x·Wᵀ plain / bias / bias + residual / GELU-D with bias; dY·W plain /
alpha / multiply-backward.  Forms only the generic instance takes: residual alone, accumulate, residual +
accumulate, alpha on x·Wᵀ, bias + alpha, fp32 output, GELU, GELU-backward, the other two layouts.
The non-temporal store form cannot be forced from the binding; one output over the 1 GiB threshold runs it.
"""

import contextlib

import exact_ints as E
import pytest
import torch
from replicann_amd import ops

pytestmark = pytest.mark.gpu

TAILS = [(1, 264), (255, 264), (257, 264), (385, 264), (257, 8), (257, 40), (257, 392)]
DEPTHS = [pytest.param(64, 0, id="K64"), pytest.param(320, 0, id="K320-static"), pytest.param(320, 1, id="K320-dynamic")]
CFG = 9


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_problems():
    yield
    E.clear_caches()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def schedule(sched):
    torch.ops.replicann.gemm_set_sched(sched)
    try:
        yield
    finally:
        torch.ops.replicann.gemm_set_sched(0)


def offset_view(M, N, device, dtype=torch.bfloat16):
    """Columns [8, 8 + N) of a sentinel-filled [M + 8][N + 24] buffer (N % 8 == 0: 16-byte rows)."""
    big = torch.full((M + 8, N + 24), E.SENTINEL, device=device, dtype=dtype)
    return big, big[:M, 8:8 + N]


def outside_untouched(big, M, N):
    rest = big.clone()
    rest[:M, 8:8 + N] = E.SENTINEL
    return bool((rest == E.SENTINEL).all())


@pytest.mark.parametrize("K,sched", DEPTHS)
@pytest.mark.parametrize("M,N", TAILS)
def test_plain_all_layouts(cuda, M, N, K, sched):
    with schedule(sched):
        for ta, tb in E.LAYOUTS:
            E.case_plain(cuda, M, N, K, ta, tb, cfgs=(CFG,), view_cfgs=(CFG,))
            a, b, exp = E.plain_problem(str(cuda), M, N, K, ta, tb)
            big, view = offset_view(M, N, cuda)
            ops.gemm(a, b, ta=ta, tb=tb, cfg=CFG, out=view)
            E.assert_bitwise(view, exp, what=f"ta {ta} tb {tb} into columns [8, 8 + N)")
            assert outside_untouched(big, M, N), f"ta {ta} tb {tb}: wrote outside the out view"


@pytest.mark.parametrize("K,sched", DEPTHS)
@pytest.mark.parametrize("M,N", TAILS)
def test_epilogue_forms(cuda, M, N, K, sched):
    """Every sum below is an integer below 2^24 (or a power-of-two multiple of one): exact in fp32 in any
    order, so each output is the one rounding of the float64 value (exact_ints.case_residual, form "once")."""
    a, b, bias, res, acc32, h = E.epilogue_problem(str(cuda), M, N, K)
    out0 = E.int_operand((M, N), -128, 128, device=cuda, generator=E.gen(3 + M + N + K))
    b64, r64, o64 = bias.double(), res.double(), out0.double()
    bt = b.t().contiguous()  # the dY·W layout of the same product
    E.require_rounding(h + b64, h + b64 + r64, h + r64, h + o64, h + r64 + o64, 0.25 * h, 2.0 * h + b64)
    miss = E.Misses()
    with schedule(sched):
        miss.check("bias", ops.gemm(a, b, tb=True, bias=bias, cfg=CFG), E.expect_bf16(h + b64))
        miss.check("bias + residual", ops.gemm(a, b, tb=True, bias=bias, residual=res, cfg=CFG), E.expect_bf16(h + b64 + r64))
        miss.check("residual", ops.gemm(a, b, tb=True, residual=res, cfg=CFG), E.expect_bf16(h + r64))
        out = out0.clone()
        ops.gemm(a, b, tb=True, out=out, accumulate=True, cfg=CFG)
        miss.check("accumulate bf16", out, E.expect_bf16(h + o64))
        out = out0.clone()
        ops.gemm(a, b, tb=True, residual=res, out=out, accumulate=True, cfg=CFG)
        miss.check("residual + accumulate", out, E.expect_bf16(h + r64 + o64))
        acc = acc32.clone()
        ops.gemm(a, b, tb=True, out=acc, accumulate=True, cfg=CFG)
        miss.check("accumulate fp32", acc, (acc32.double() + h).float())
        miss.check("fp32 out", ops.gemm(a, b, tb=True, out_dtype=torch.float32, cfg=CFG), h.float())
        for v in (0.25, 2.0):  # a power of two scales exactly
            al = torch.tensor([v], device=cuda)
            miss.check(f"alpha {v}", ops.gemm(a, b, tb=True, alpha=al, cfg=CFG), E.expect_bf16(v * h))
            miss.check(f"alpha {v}, dY·W", ops.gemm(a, bt, alpha=al, cfg=CFG), E.expect_bf16(v * h))
            miss.check(f"bias + alpha {v}", ops.gemm(a, b, tb=True, bias=bias, alpha=al, cfg=CFG), E.expect_bf16(v * h + b64))
        # bias and bias + residual into a view with a row stride > N
        big, view = offset_view(M, N, cuda)
        ops.gemm(a, b, tb=True, bias=bias, cfg=CFG, out=view)
        miss.check("bias into a view", view, E.expect_bf16(h + b64))
        miss.check_true("bias into a view", outside_untouched(big, M, N), "wrote outside the out view")
        big, view = offset_view(M, N, cuda)
        rbig, rview = offset_view(M, N, cuda)
        rview.copy_(res)
        ops.gemm(a, b, tb=True, bias=bias, residual=rview, cfg=CFG, out=view)
        miss.check("bias + residual into a view", view, E.expect_bf16(h + b64 + r64))
        miss.check_true("bias + residual into a view", outside_untouched(big, M, N), "wrote outside the out view")
    miss.done()


def test_non_temporal_form(cuda):
    """The non-temporal store form runs only for bf16 outputs over 1 GiB (rn_gemm_st_nt) and the binding has no
    switch for it, so one such output: 16385 x 32776 (a one-row M tail, an 8-column N tail in the left half),
    K = 64.  The float64 reference is formed and compared 2048 rows at a time."""
    M, N, K = 16385, 32776, 64
    assert M * N * 2 > 1 << 30
    g = E.gen(5)
    h = E.rounding_hi(K)
    a = E.int_operand((M, K), -h, h, device=cuda, generator=g)
    b = E.int_operand((N, K), -h, h, device=cuda, generator=g)
    out = ops.gemm(a, b, tb=True, cfg=CFG)
    b64 = b.double().t()
    for r0 in range(0, M, 2048):
        ref = a[r0:r0 + 2048].double() @ b64
        if r0 == 0:
            E.require_rounding(ref)
        E.assert_bitwise(out[r0:r0 + 2048], E.expect_bf16(ref), what=f"non-temporal stores, rows {r0}..")
    del out, ref, b64
    torch.cuda.empty_cache()


def gelu_bwd_problem(device, M, N, K):
    """Code 4 with an exact expected value: a saved pre-activation in {0, 8}, where the tanh-GELU derivative is
    0.5 and (the sigmoid saturated: 2^-71 below 1) 1 in fp32 and in float64 alike.  dH is then the integer
    product or half of it, a bf16 value while the product stays within 128 (asserted): the representable class
    of group c; K = 320 draws a thinner operand for it."""
    g = E.gen(43 + 1000 * M + 10 * N + K)
    dens = 1.0 if K <= 64 else 0.25
    a = E.int_operand((M, K), -1, 1, density=dens, device=device, generator=g)
    b = E.int_operand((K, N), -1, 1, density=dens, device=device, generator=g)
    pre = 8 * E.int_operand((M, N), 0, 1, device=device, generator=g)
    bg0 = E.int_operand((N,), -9, 9, device=device, generator=g)
    du = a.double() @ b.double()
    out = du * torch.where(pre.double() > 0, 1.0, 0.5)
    E.require_representable(du, 2 * out)
    assert float(out.abs().sum(0).max()) + 9 < E.F32_EXACT_INT / 2  # every order of the column sum is exact
    return a, b, pre, bg0, E.expect_bf16(out), E.expect_bf16(bg0.double() + out.sum(0))


@pytest.mark.parametrize("K,sched", DEPTHS)
@pytest.mark.parametrize("M,N", TAILS)
def test_act_bwd_bias_grad(cuda, M, N, K, sched):
    """dH and the bias gradient from the column partials, bit for bit: code 6 as group c of
    test_gemm_exact_gpu.py does it (contiguous and into a strided view), code 4 on gelu_bwd_problem."""
    with schedule(sched):
        E.case_act_bwd(cuda, M, N, K, 6, variants=((CFG, 0),), strided=((CFG, 0, 16),))
        a, b, pre, bg0, exp, exp_bg = gelu_bwd_problem(str(cuda), M, N, K)
        miss = E.Misses(zero_sign=False)
        bg = bg0.clone()
        out = E.gemm_bwd(a, b, 4, pre, bias_grad=bg, cfg=CFG)
        miss.check("act 4: out", out, exp)
        miss.check("act 4: bias_grad", bg.view(1, -1), exp_bg.view(1, -1))
        big, view = offset_view(M, N, cuda)
        pbig, pview = offset_view(M, N, cuda)
        pview.copy_(pre)
        bg = bg0.clone()
        E.gemm_bwd(a, b, 4, pview, out=view, bias_grad=bg, cfg=CFG)
        miss.check("act 4 into a view: out", view, exp)
        miss.check("act 4 into a view: bias_grad", bg.view(1, -1), exp_bg.view(1, -1))
        miss.check_true("act 4 into a view", outside_untouched(big, M, N), "wrote outside the out view")
        miss.done()


@pytest.mark.parametrize("K,sched", DEPTHS)
@pytest.mark.parametrize("M,N", TAILS)
def test_gelu_forward(cuda, M, N, K, sched):
    """GELU (code 2) and saved-derivative GELU (code 5): the pre-activation bitwise, gelu(h) and gelu'(h)
    within exact_ints.gelu_report's per-element bound."""
    with schedule(sched):
        E.case_gelu(cuda, M, N, K, 1.0 if K <= 64 else 0.5, cfgs=(CFG,))
