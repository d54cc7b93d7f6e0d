"""Exact GEMM checks on integer operands: generators, expected values, a bitwise comparison, the cases.

bf16 and fp8 MFMAs form exact products and accumulate in fp32.  With small integer operands every partial
sum is an integer below 2^24, so the fp32 result is exact whatever the accumulation order, tile shape,
split-K or one-hot-MFMA residual; the only inexact step of a kernel is its final round-to-nearest-even to
bf16.  The expected output is therefore known bit for bit, and every tile config must produce it.

Two operand classes:
  representable  A, B in {-1, 0, 1}: every intermediate is an integer <= 256 and exact in bf16 too (a rounded
                 pre-activation, a bf16 accumulate target); the cases assert max|.| <= 256 on their reference.
  rounding       A, B in {-h .. h}: a share of the outputs is not a bf16 value, so the final rounding is
                 exercised; the cases assert max|.| < 2^24 and that >= 0.1 % of the outputs round.

The case functions run on either device: on CPU tensors ``ops.gemm`` is fp32 ATen math, exact on these
operands, which checks every generator, precondition and expected-value formula without a GPU
(tests/test_exact_ints.py); tests/test_gemm_exact_gpu.py runs them against the HIP kernels.
A plain module, not a conftest.
"""

import functools
import math

import torch
import torch.nn.functional as F

from replicann_amd import _ext, ops
from replicann_amd.ops.linear import ACT_GELU, ACT_GELU_D, ACT_RELU, bias_act_grad

BF16_EXACT_INT = 256  # every integer of magnitude <= 2^8 is a bf16 value (8 significand bits)
F32_EXACT_INT = 1 << 24


# (M, N, K).  Ragged single and multi tile; N % 8 != 0 (cfg 9 runs cfg 1's kernel, the binding forces a
# transpose), K % 8 != 0 (the zero-pad path) and M % 8 != 0 (an M-contiguous A is transposed); more than 256
# tiles of 256x256, so the persistent kernels walk >= 2 tiles per workgroup: K = 72 and 128 are shorter than
# the 6-half-tile lookahead, 128 is nk = 2 (the tightest wait counts of cfg 11), 384 is 6 K-tiles (its
# residual bodies).
RAGGED = [(200, 72, 96), (64, 24, 8), (1000, 384, 520), (520, 776, 1088)]
ODD = [(203, 76, 100), (300, 203, 515)]
PERSISTENT = [(8200, 2056, 72), (8200, 2056, 128), (8200, 2056, 384)]
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]  # (ta, tb)
SKINNY = [(M, N, K) for M in (1, 5, 33, 64) for N, K in ((776, 1088), (200, 520))]
# partial last 128-row and 256-row tiles: rows >= M must contribute nothing to the bias gradient
ACT_BWD = [(4600, 3072, 72), (300, 264, 192)]
# more than 1024 column-partial rows (gemm_plan.h gemm_colpart_rows: cfg 9 writes two per 256-row tile, 1028 here;
# the 128-row configs 1027), the first size at which the column reduction is the ticketed rn_colsum_k and not the
# one-block rn_colsum1_k.  K = 8: |a·b| <= 8, the column sums stay below 8 · 131400 < 2^24
ACT_BWD_TICKET = (131400, 72, 8)
# (M, N, K, density): |h| <= 64 needs a thinner operand at K = 520
GELU = [(200, 72, 96, 1.0), (1000, 384, 520, 0.5), (8200, 2056, 72, 1.0)]
FP8_FWD = [(1000, 776, 512), (8200, 2056, 2048)]  # the second takes the K >= 2048 persistent path
FP8_DGRAD = [(1000, 784, 512)]  # N and K multiples of 16
FP8_WGRAD = [(272, 144, 1024)]  # M, N multiples of 16, K (tokens) of 128
# (C, OC, k, S, P, HW): the halo kernel; the implicit GEMM; col2im for dgrad; 128 input channels
CONV = [(64, 64, 3, 1, 1, 16), (64, 64, 3, 1, 1, 14), (64, 128, 3, 2, 1, 15), (128, 64, 3, 1, 1, 9)]


# ------------------------------------------------------------------------------------------------
# generators and expected values
# ------------------------------------------------------------------------------------------------
def int_operand(shape, lo, hi, density=1.0, dtype=torch.bfloat16, device="cpu", generator=None):
    """Integers drawn uniformly from {lo .. hi}; each kept with probability ``density``, else 0.  Drawn on
    the CPU (the same values on both tiers), then moved."""
    v = torch.randint(lo, hi + 1, tuple(shape), generator=generator, dtype=torch.int32)
    if density < 1.0:
        v = v * (torch.rand(tuple(shape), generator=generator) < density)
    assert max(abs(lo), abs(hi)) <= (BF16_EXACT_INT if dtype == torch.bfloat16 else F32_EXACT_INT)
    return v.to(dtype).to(device)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def expect_bf16(ref64):
    """The one round-to-nearest-even of an exact float64 reference."""
    assert ref64.dtype == torch.float64
    return ref64.to(torch.bfloat16)


def rounding_hi(K):
    """The operand range {-h .. h} of the rounding class for a K-deep sum: the smallest h >= 4 at which the
    standard deviation of the sum, h(h+1)/3 · sqrt(K), reaches 128.  Then |sum| > 256, where half of the
    integers are no bf16 value, is a two-sigma event (a few per cent of the outputs).  h = 4 from K = 370
    up; shorter sums need wider operands to round at all (K = 8: |sum| <= 128 with h = 4)."""
    h = 4
    while h * (h + 1) / 3.0 * math.sqrt(K) < 128 and h < 16:
        h += 1
    return h


def require_representable(*tensors):
    for t in tensors:
        m = float(t.abs().max())
        assert m <= BF16_EXACT_INT, f"precondition: max|intermediate| = {m} > {BF16_EXACT_INT}"


def require_rounding(*refs64):
    """Every value exact in fp32; over all given outputs at least 0.1 % change in the bf16 rounding."""
    n = diff = 0
    for r in refs64:
        assert float(r.abs().max()) < F32_EXACT_INT
        n += r.numel()
        diff += int((r.to(torch.bfloat16).double() != r).sum())
    assert diff >= 1e-3 * n, f"precondition: only {diff} of {n} outputs need the final rounding"


# ------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------
def _bits(t, zero_sign):
    t = t.detach()
    if not zero_sign:  # x + 0 is +0 for both zeros, every other value is unchanged
        t = t + 0
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16)
    assert t.dtype == torch.float32, t.dtype
    return t.view(torch.int32)


def bitwise_report(out, expected, tile=(256, 256), zero_sign=True):
    """None if ``out`` equals ``expected`` bit for bit in every element, else the report of the misses.
    The raw bits, so -0 is not +0; ``zero_sign=False`` lets the two zeros agree, for the activation-backward
    cases alone: there 0 times a negative sum is -0 as a product and +0 as a select, and neither is wrong."""
    assert out.shape == expected.shape, (tuple(out.shape), tuple(expected.shape))
    assert out.dtype == expected.dtype, (out.dtype, expected.dtype)
    o2 = out.reshape(-1, out.shape[-1]) if out.dim() != 2 else out
    e2 = expected.reshape(-1, expected.shape[-1]) if expected.dim() != 2 else expected
    bad = _bits(o2, zero_sign) != _bits(e2.to(o2.device), zero_sign)
    n = int(bad.sum())
    if n == 0:
        return None
    idx = bad.nonzero()
    r, c = (int(v) for v in idx[0])
    tiles = sorted({(int(a), int(b)) for a, b in torch.stack([idx[:, 0] // tile[0], idx[:, 1] // tile[1]], 1)
                    .unique(dim=0).tolist()})
    r0, c0 = r // 16 * 16, c // 16 * 16
    box_o = o2[r0:r0 + 16, c0:c0 + 16].float().cpu()
    box_e = e2[r0:r0 + 16, c0:c0 + 16].float().cpu()
    shown = tiles if len(tiles) <= 24 else tiles[:24] + ["..."]
    return (f"{n} of {bad.numel()} elements differ; first at ({r}, {c}): got {float(o2[r, c])!r}, expected "
            f"{float(e2[r, c])!r}\n{tile[0]}x{tile[1]} tiles (row, col) affected: {len(tiles)}: {shown}\n"
            f"16x16 box at rows {r0}.., cols {c0}..\n got:\n{box_o}\n expected:\n{box_e}")


def assert_bitwise(out, expected, tile=(256, 256), what="", zero_sign=True):
    rep = bitwise_report(out, expected, tile, zero_sign)
    assert rep is None, f"{what}: {rep}" if what else rep


class Misses:
    """Collects the reports of one case over its configs, so that one run names every config that is wrong."""

    def __init__(self, zero_sign=True):
        self.reports, self.zero_sign = [], zero_sign

    def check(self, what, out, expected):
        rep = bitwise_report(out, expected, zero_sign=self.zero_sign)
        if rep is not None:
            self.reports.append(f"[{what}] {rep}")

    def check_true(self, what, ok, msg):
        if not ok:
            self.reports.append(f"[{what}] {msg}")

    def done(self):
        assert not self.reports, f"{len(self.reports)} config(s) wrong:\n" + "\n\n".join(self.reports)


# ------------------------------------------------------------------------------------------------
# the op under test
# ------------------------------------------------------------------------------------------------
def w1_takes(M, N, K, ta, tb, ldc=None):
    """Does cfg 11 take the plain bf16 problem?  The library's own answer (gemm_cfg_takes(11, ...) of
    csrc/include/gemm_plan.h through the debug op gemm_candidates), for the problem as the binding makes it
    canonical: K padded to 8, an A or B whose contiguous dimension is no multiple of 8 transposed."""
    Kp = (K + 7) // 8 * 8
    ta, tb = ta and M % 8 == 0, tb or N % 8 != 0
    flat = torch.ops.replicann.gemm_candidates(M, N, Kp, ta, tb, 0, False, False, 0, False, False, False, False,
                                               ldc or N)
    return 11 in flat[0::2]


def gemm_bwd(a, b, act, preact, out=None, bias_grad=None, split_k=0, cfg=-1):
    """The activation-backward GEMM, out = (a·b) ⊙ act'(preact), with the fused bias gradient
    (bias_grad += Σ_rows out).  GPU: the native op.  CPU: the same math in fp32 (ops.gemm's CPU path has
    act 6 only and no bias gradient)."""
    if _ext.use_native(a):
        return torch.ops.replicann.gemm(a, b, False, False, None, None, act, preact, out, False, split_k, False, None,
                                        cfg, bias_grad)
    du = a.float() @ b.float()
    if act == 3:
        y = du * (preact.float() > 0)
    elif act == 4:
        y = (du.double() * gelu_grad64(preact.double())).float()
    else:
        assert act == 6
        y = du * preact.float()
    y = y.to(torch.bfloat16)
    if bias_grad is not None:
        bias_grad.copy_((bias_grad.float() + y.float().sum(0)).to(torch.bfloat16))
    if out is not None:
        out.copy_(y)
        return out
    return y


SENTINEL = 7.0


def sentinel_view(M, N, device, dtype=torch.bfloat16, extra=16):
    """An [M][N] view of a larger buffer filled with a sentinel; its row stride is N rounded up to 8 plus
    ``extra`` (16: a multiple of 8; 4: none, but still 8-byte rows)."""
    big = torch.full((M + 8, (N + 7) // 8 * 8 + extra), SENTINEL, device=device, dtype=dtype)
    return big, big[:M, :N]


def outside_untouched(big, M, N):
    return bool((big[M:] == SENTINEL).all()) and bool((big[:, N:] == SENTINEL).all())


def clear_caches():
    """Drop the shared problems (operands and float64 references); the test modules call it at teardown."""
    for f in (epilogue_problem, bwd_problem, fp8_fwd_problem):
        f.cache_clear()


# ------------------------------------------------------------------------------------------------
# group a: the plain product
# ------------------------------------------------------------------------------------------------
TILE_CFGS = (0, 1, 2, 3, 4, 5, 6, 8, 9, -1)


def plain_problem(device, M, N, K, ta, tb):
    """(a, b, expected bf16) of the rounding class, shared by the configs of one case."""
    g = gen(1000 * M + 10 * N + K + 2 * ta + tb)
    h = rounding_hi(K)
    a = int_operand((K, M) if ta else (M, K), -h, h, device=device, generator=g)
    b = int_operand((N, K) if tb else (K, N), -h, h, device=device, generator=g)
    A, B = (a.t() if ta else a).double(), (b.t() if tb else b).double()
    ref = A @ B
    require_rounding(ref)
    return a, b, expect_bf16(ref)


def case_plain(device, M, N, K, ta, tb, cfgs=TILE_CFGS, view_cfgs=()):
    a, b, exp = plain_problem(str(device), M, N, K, ta, tb)
    miss = Misses()
    for cfg in cfgs:
        miss.check(f"cfg {cfg}", ops.gemm(a, b, ta=ta, tb=tb, cfg=cfg), exp)
    for cfg in view_cfgs:  # an out view of a larger buffer: everything outside it stays
        big, view = sentinel_view(M, N, device)
        ops.gemm(a, b, ta=ta, tb=tb, cfg=cfg, out=view)
        miss.check(f"cfg {cfg} into a view", view, exp)
        miss.check_true(f"cfg {cfg} into a view", outside_untouched(big, M, N), "wrote outside the out view")
    miss.done()


def case_skinny(device, M, N, K, splits=(0, 2, 3)):
    """cfg 10, the skinny-M decode GEMM (x·Wᵀ, M <= 64); split_k = K ranges."""
    a, b, exp = plain_problem(str(device), M, N, K, False, True)
    miss = Misses()
    for sk in splits:
        miss.check(f"cfg 10 split_k {sk}", ops.gemm(a, b, tb=True, cfg=10, split_k=sk), exp)
    miss.done()


# ------------------------------------------------------------------------------------------------
# group b: epilogues that stay exact (x·Wᵀ layout)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def epilogue_problem(device, M, N, K):
    g = gen(7 + 1000 * M + 10 * N + K)
    h = rounding_hi(K)
    a = int_operand((M, K), -h, h, device=device, generator=g)
    b = int_operand((N, K), -h, h, device=device, generator=g)
    bias = int_operand((N,), -64, 64, device=device, generator=g)
    res = int_operand((M, N), -128, 128, device=device, generator=g)
    acc32 = int_operand((M, N), -1000, 1000, dtype=torch.float32, device=device, generator=g)
    hh = a.double() @ b.double().t()
    return a, b, bias, res, acc32, hh


def case_epilogues(device, M, N, K, cfgs=TILE_CFGS, with_w1=False):
    """Integer bias, power-of-two alpha, ReLU with its pre-activation, fp32 output, accumulate into fp32: each
    is exact before the one final rounding.  (The residual: case_residual.)"""
    a, b, bias, res, acc32, h = epilogue_problem(str(device), M, N, K)
    b64 = bias.double()
    require_rounding(h + b64, 0.25 * h, torch.relu(h + b64), acc32.double() + h)
    miss = Misses()
    alphas = {v: torch.tensor([v], device=device) for v in (0.25, 2.0)}
    w1 = [11] if with_w1 and w1_takes(M, N, K, False, True) else []
    for cfg in list(cfgs) + w1:
        tag = f"cfg {cfg}"
        miss.check(f"{tag} bias", ops.gemm(a, b, tb=True, bias=bias, cfg=cfg), expect_bf16(h + b64))
        for v, al in alphas.items():  # a power of two scales exactly
            miss.check(f"{tag} alpha {v}", ops.gemm(a, b, tb=True, alpha=al, cfg=cfg), expect_bf16(v * h))
        if cfg == 11:
            continue  # cfg 11 takes no activation, fp32 output or accumulate (it would run cfg 9 again)
        pre = torch.full((M, N), SENTINEL, device=device, dtype=torch.bfloat16)
        y = ops.gemm(a, b, tb=True, bias=bias, act=ACT_RELU, preact=pre, cfg=cfg)
        miss.check(f"{tag} relu: preact", pre, expect_bf16(h + b64))
        miss.check(f"{tag} relu: out", y, expect_bf16(torch.relu(h + b64)))
        miss.check(f"{tag} fp32 out", ops.gemm(a, b, tb=True, out_dtype=torch.float32, cfg=cfg), h.float())
        acc = acc32.clone()
        ops.gemm(a, b, tb=True, out=acc, accumulate=True, cfg=cfg)
        miss.check(f"{tag} accumulate fp32", acc, (acc32.double() + h).float())
    miss.done()


def case_residual(device, M, N, K, cfg, relu, rounds="once"):
    """An integer residual on top of bias (and of ReLU with its pre-activation), bit for bit.  Two exactly
    computable forms, both part of the kernels' contract (docs/DESIGN.md, GEMM epilogues):
      once   round(act(h + bias) + r): the direct epilogue, the split-K reduce, cfg 9 / 11 without an
             activation (and the CPU path);
      twice  round(round(act(h + bias)) + r): the epilogue staged through LDS as a bf16 tile, which adds the
             residual to the stored value of act(h + bias).
    ``rounds`` names the one form this config must give; "either" (cfg -1, where the tuner picks the config
    by time) accepts a whole output in one of the two forms.  The operands make the forms differ, so a pass
    is never a coincidence, and every element is compared in every case."""
    a, b, bias, res, acc32, h = epilogue_problem(str(device), M, N, K)
    hb, r64 = h + bias.double(), res.double()
    act64 = torch.relu(hb) if relu else hb
    forms = {"once": expect_bf16(act64 + r64), "twice": expect_bf16(expect_bf16(act64).double() + r64)}
    require_rounding(act64 + r64)
    differ = int((forms["once"] != forms["twice"]).sum())
    assert differ >= 1e-3 * h.numel(), f"precondition: the two forms differ in only {differ} elements"
    tag = f"cfg {cfg} {'relu+' if relu else 'bias+'}residual"
    if relu:
        pre = torch.full((M, N), SENTINEL, device=device, dtype=torch.bfloat16)
        y = ops.gemm(a, b, tb=True, bias=bias, residual=res, act=ACT_RELU, preact=pre, cfg=cfg)
        assert_bitwise(pre, expect_bf16(hb), what=f"{tag}: preact")
    else:
        y = ops.gemm(a, b, tb=True, bias=bias, residual=res, cfg=cfg)
    if rounds == "either":
        reps = {k: bitwise_report(y, v) for k, v in forms.items()}
        assert None in reps.values(), f"{tag}: neither form.\nvs once: {reps['once']}\nvs twice: {reps['twice']}"
    else:
        assert_bitwise(y, forms[rounds], what=f"{tag} (rounded {rounds})")


def case_split_k(device, M, N, K, cfgs=(0, 1, 9, -1), splits=(2, 3, 7)):
    """Explicit split-K: fp32 slabs summed in fixed order, then the epilogue; exact for any split."""
    a, b, bias, res, acc32, h = epilogue_problem(str(device), M, N, K)
    exp = expect_bf16(h + bias.double() + res.double())
    require_rounding(h + bias.double() + res.double())
    miss = Misses()
    for cfg in cfgs:
        for sk in splits:
            miss.check(f"cfg {cfg} split_k {sk}", ops.gemm(a, b, tb=True, bias=bias, residual=res, cfg=cfg, split_k=sk),
                       exp)
            acc = acc32.clone()
            ops.gemm(a, b, tb=True, out=acc, accumulate=True, cfg=cfg, split_k=sk)
            miss.check(f"cfg {cfg} split_k {sk} accumulate fp32", acc, (acc32.double() + h).float())
    miss.done()


def case_accumulate_bf16(device, M, N, K, cfgs=TILE_CFGS):
    """accumulate into a bf16 out: whether the kernel rounds the product before the add is not part of the
    contract, so the representable class, where both orders give the same exact integer."""
    g = gen(11 + M + N + K)
    a = int_operand((M, K), -1, 1, device=device, generator=g)
    b = int_operand((N, K), -1, 1, device=device, generator=g)
    out0 = int_operand((M, N), -64, 64, device=device, generator=g)
    h = a.double() @ b.double().t()
    require_representable(h, out0.double() + h)
    exp = expect_bf16(out0.double() + h)
    miss = Misses()
    for cfg in cfgs:
        out = out0.clone()
        ops.gemm(a, b, tb=True, out=out, accumulate=True, cfg=cfg)
        miss.check(f"cfg {cfg} accumulate bf16", out, exp)
    miss.done()


# ------------------------------------------------------------------------------------------------
# group c: activation-backward epilogues with the fused bias gradient (dgrad layout, representable class)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def bwd_problem(device, M, N, K, act):
    g = gen(13 + 1000 * M + 10 * N + K + act)
    a = int_operand((M, K), -1, 1, device=device, generator=g)
    b = int_operand((K, N), -1, 1, device=device, generator=g)
    # act 3 (ReLU'): integers of random sign with exact zeros; act 6 (multiply): {-1, 0, 1}
    pre = int_operand((M, N), -3, 3, density=0.8, device=device, generator=g) if act == 3 else \
        int_operand((M, N), -1, 1, device=device, generator=g)
    bg0 = int_operand((N,), -9, 9, device=device, generator=g)
    du = a.double() @ b.double()
    out = du * (pre.double() > 0) if act == 3 else du * pre.double()
    bg = bg0.double() + out.sum(0)
    require_representable(du, out)
    assert float(out.abs().sum(0).max()) + 9 < F32_EXACT_INT  # every order of the column sum is exact
    assert bool((pre == 0).any()) and bool((pre < 0).any()) and bool((pre > 0).any())
    return a, b, pre, bg0, expect_bf16(out), expect_bf16(bg)


# (cfg, split_k): configs that emit column partials; configs that cannot, where the binding reduces the
# output itself; and requests that are not the config that runs (-1 with an explicit split runs cfg 9,
# which writes two partial rows per 256-row tile; so does an 11, which takes no activation backward)
BWD_COLPART = ((0, 0), (1, 0), (2, 0), (5, 0), (8, 0), (9, 0))
BWD_REDUCE = ((3, 0), (4, 0), (6, 0), (9, 3))
BWD_UNRESOLVED = ((-1, 1), (11, 0))


# (cfg, split_k, extra row stride): an out view with a row stride > N, preact with the same stride.  16: a
# multiple of 8 (cfg 3 reduces the output itself, cfg 9 emits column partials); 4: no multiple of 8, where
# every config reduces the output itself, by the reduction's scalar path
BWD_STRIDED = ((3, 0, 16), (9, 0, 16), (1, 0, 4), (9, 0, 4))


def case_act_bwd(device, M, N, K, act, variants=BWD_COLPART + BWD_REDUCE + BWD_UNRESOLVED, strided=BWD_STRIDED):
    a, b, pre, bg0, exp, exp_bg = bwd_problem(str(device), M, N, K, act)
    miss = Misses(zero_sign=False)  # 0 · (a negative sum) is -0 as a product, +0 as a select
    for cfg, sk in variants:
        bg = bg0.clone()
        out = gemm_bwd(a, b, act, pre, bias_grad=bg, split_k=sk, cfg=cfg)
        miss.check(f"cfg {cfg} split_k {sk}: out", out, exp)
        miss.check(f"cfg {cfg} split_k {sk}: bias_grad", bg.view(1, -1), exp_bg.view(1, -1))
    for cfg, sk, extra in strided:
        big, view = sentinel_view(M, N, device, extra=extra)
        pbig, pview = sentinel_view(M, N, device, extra=extra)
        pview.copy_(pre)
        bg = bg0.clone()
        gemm_bwd(a, b, act, pview, out=view, bias_grad=bg, split_k=sk, cfg=cfg)
        tag = f"cfg {cfg} split_k {sk} out with row stride {view.stride(0)}"
        miss.check(f"{tag}: out", view, exp)
        miss.check(f"{tag}: bias_grad", bg.view(1, -1), exp_bg.view(1, -1))
        miss.check_true(tag, outside_untouched(big, M, N), "wrote outside the out view")
    miss.done()


def case_bias_grad_unaligned(device, M, N):
    """The bias-gradient reduction (ops.bias_act_grad, act none) of a contiguous dy whose first element is
    not 16-byte aligned: 16-byte row loads are not possible, the scalar path sums it."""
    g = gen(41 + M + N)
    flat = int_operand((M * N + 3,), -64, 64, device=device, generator=g)
    dy = flat[3:].view(M, N)
    assert dy.is_contiguous() and dy.data_ptr() % 16 != 0
    exp = dy.double().sum(0)
    require_representable(dy)
    assert float(dy.double().abs().sum(0).max()) < F32_EXACT_INT
    _, db = bias_act_grad(dy, None, 0, True)
    assert_bitwise(db.to(torch.bfloat16).view(1, -1), expect_bf16(exp).view(1, -1), what="bias_act_grad, unaligned dy")


# ------------------------------------------------------------------------------------------------
# group d: GELU epilogues (representable class, |h| <= 64)
# ------------------------------------------------------------------------------------------------
_C = math.sqrt(2.0 / math.pi)


def gelu64(h):
    return 0.5 * h * (1 + torch.tanh(_C * (h + 0.044715 * h**3)))


def gelu_grad64(h):
    t = torch.tanh(_C * (h + 0.044715 * h**3))
    return 0.5 * (1 + t) + 0.5 * h * (1 - t * t) * _C * (1 + 3 * 0.044715 * h * h)


def gelu_report(got, g64):
    """Per element |got - g| <= 2^-7·|g| + 2^-16, g the float64 tanh-GELU (or its derivative) at the exact h.
    One bf16 rounding is at most 2^-8 relative; the other 2^-8 is the margin for the fp32 evaluation; the
    absolute term covers the cancellation in 1 + tanh: 2^-24 · 4 · max|h| with max|h| <= 64.  Elementwise,
    not a norm: one wrong element fails.  None, or the report of the elements over the bound."""
    err = (got.double() - g64).abs()
    bad = err > 2.0**-7 * g64.abs() + 2.0**-16
    n = int(bad.sum())
    if n == 0:
        return None
    idx = bad.nonzero()
    r, c = (int(v) for v in idx[0])
    worst = (err - 2.0**-7 * g64.abs() - 2.0**-16).argmax()
    wr, wc = int(worst) // got.shape[1], int(worst) % got.shape[1]
    return (f"{n} of {bad.numel()} elements over the bound; first at ({r}, {c}): got {float(got[r, c])!r}, "
            f"float64 {float(g64[r, c])!r}; worst at ({wr}, {wc}): got {float(got[wr, wc])!r}, float64 "
            f"{float(g64[wr, wc])!r}")


def case_gelu(device, M, N, K, density, cfgs=TILE_CFGS):
    g = gen(17 + M + N + K)
    a = int_operand((M, K), -1, 1, density=density, device=device, generator=g)
    b = int_operand((N, K), -1, 1, density=density, device=device, generator=g)
    bias = int_operand((N,), -2, 2, device=device, generator=g)
    h = a.double() @ b.double().t() + bias.double()
    assert float(h.abs().max()) <= 64, float(h.abs().max())
    eh, g64, d64 = expect_bf16(h), gelu64(h), gelu_grad64(h)
    miss = Misses()
    for cfg in cfgs:
        pre = torch.full((M, N), SENTINEL, device=device, dtype=torch.bfloat16)
        y = ops.gemm(a, b, tb=True, bias=bias, act=ACT_GELU, preact=pre, cfg=cfg)
        miss.check(f"cfg {cfg} act 2: preact", pre, eh)
        rep = gelu_report(y, g64)
        miss.check_true(f"cfg {cfg} act 2: out", rep is None, rep)
        d = torch.full((M, N), SENTINEL, device=device, dtype=torch.bfloat16)
        y = ops.gemm(a, b, tb=True, bias=bias, act=ACT_GELU_D, preact=d, cfg=cfg)
        rep = gelu_report(y, g64)
        miss.check_true(f"cfg {cfg} act 5: out", rep is None, rep)
        rep = gelu_report(d, d64)
        miss.check_true(f"cfg {cfg} act 5: saved gelu'", rep is None, rep)
    miss.done()


def case_gelu_bwd(device, M, N, K, density, cfgs=TILE_CFGS):
    """act 4: out = (a·b) ⊙ gelu'(pre), the product exact, pre integer-valued."""
    g = gen(19 + M + N + K)
    a = int_operand((M, K), -1, 1, density=density, device=device, generator=g)
    b = int_operand((K, N), -1, 1, density=density, device=device, generator=g)
    pre = int_operand((M, N), -6, 6, device=device, generator=g)
    du = a.double() @ b.double()
    assert float(du.abs().max()) <= 64 and float(pre.abs().max()) <= 64
    ref = du * gelu_grad64(pre.double())
    miss = Misses()
    for cfg in cfgs:
        rep = gelu_report(gemm_bwd(a, b, 4, pre, cfg=cfg), ref)
        miss.check_true(f"cfg {cfg} act 4: out", rep is None, rep)
    miss.done()


# ------------------------------------------------------------------------------------------------
# group e: fp8
# ------------------------------------------------------------------------------------------------
def is_pow2(s):
    m, _ = torch.frexp(s.detach().float().cpu())
    return float(m) == 0.5


def quant_e4m3(x):
    """The project's e4m3 quantiser on integers in {-4 .. 4}; precondition: it is lossless on them."""
    q, s = ops.quantize_fp8(x)
    assert is_pow2(s[0]), float(s[0])
    assert_bitwise(ops.dequantize_fp8(q, s), x, what="e4m3 round trip")
    return q, s


def quant_e5m2(x):
    s = torch.zeros(4, device=x.device)
    q = ops.quantize_bf8(x, s, False)
    assert is_pow2(s[0]), float(s[0])
    assert_bitwise(ops.dequantize_bf8(q, s), x, what="e5m2 round trip")
    return q, s


def fp8_operands(device, rows_a, rows_b, depth, seed, deep_first=False):
    """Integer operands in {-4 .. 4} (exact in e4m3 and e5m2) sharing ``depth``, as [rows][depth] or,
    ``deep_first``, [depth][rows]."""
    g = gen(seed)
    sa, sb = ((depth, rows_a), (depth, rows_b)) if deep_first else ((rows_a, depth), (rows_b, depth))
    return int_operand(sa, -4, 4, device=device, generator=g), int_operand(sb, -4, 4, device=device, generator=g), g


@functools.lru_cache(maxsize=1)
def fp8_fwd_problem(device, M, N, K):
    x, w, g = fp8_operands(device, M, N, K, 29 + M + N + K)
    bias = int_operand((N,), -64, 64, device=device, generator=g)
    res = int_operand((M, N), -128, 128, device=device, generator=g)
    return x, w, bias, res, quant_e4m3(x), quant_e4m3(w), x.double() @ w.double().t()


def _gemm_fp8(qa, sa, qb, sb, bias, res):
    if _ext.use_native(qa):
        return torch.ops.replicann.gemm_fp8(qa, qb, sa, sb, bias, res, 0, None)
    hf = ops.dequantize_fp8(qa, sa).float() @ ops.dequantize_fp8(qb, sb).float().t()  # the CPU emulation
    for t in (bias, res):
        hf = hf if t is None else hf + t.float()
    return hf.to(torch.bfloat16)


def case_fp8_fwd(device, M, N, K, modes=("11", "9", "0"), setenv=lambda k, v: None):
    """gemm_fp8 (x·Wᵀ, e4m3 × e4m3), plain and with bias, under each REPLICANN_FP8_GEMM kernel: the exact
    value, hence the same bits from all of them."""
    x, w, bias, res, (qa, sa), (qb, sb), h = fp8_fwd_problem(str(device), M, N, K)
    require_rounding(h, h + bias.double())
    miss = Misses()
    for mode in modes:
        setenv("REPLICANN_FP8_GEMM", mode)
        miss.check(f"REPLICANN_FP8_GEMM={mode} plain", _gemm_fp8(qa, sa, qb, sb, None, None), expect_bf16(h))
        miss.check(f"REPLICANN_FP8_GEMM={mode} bias", _gemm_fp8(qa, sa, qb, sb, bias, None),
                   expect_bf16(h + bias.double()))
    miss.done()


def case_fp8_residual(device, M, N, K, mode, setenv=lambda k, v: None, rounds="once"):
    """gemm_fp8 with bias and residual: the form (case_residual) this REPLICANN_FP8_GEMM kernel must give."""
    x, w, bias, res, (qa, sa), (qb, sb), h = fp8_fwd_problem(str(device), M, N, K)
    hb, r64 = h + bias.double(), res.double()
    forms = {"once": expect_bf16(hb + r64), "twice": expect_bf16(expect_bf16(hb).double() + r64)}
    require_rounding(hb + r64)
    differ = int((forms["once"] != forms["twice"]).sum())
    assert differ >= 1e-3 * h.numel(), f"precondition: the two forms differ in only {differ} elements"
    setenv("REPLICANN_FP8_GEMM", mode)
    assert_bitwise(_gemm_fp8(qa, sa, qb, sb, bias, res), forms[rounds],
                   what=f"REPLICANN_FP8_GEMM={mode} bias+residual (rounded {rounds})")


def case_fp8_dgrad(device, M, N, K, a_bf8):
    """gemm_fp8_dgrad: dY [M][K] (e5m2 or e4m3) · W [K][N] (e4m3, N-contiguous)."""
    g = gen(31 + M + N + K)
    a = int_operand((M, K), -4, 4, device=device, generator=g)
    b = int_operand((K, N), -4, 4, device=device, generator=g)
    qa, sa = quant_e5m2(a) if a_bf8 else quant_e4m3(a)
    qb, sb = quant_e4m3(b)
    ref = a.double() @ b.double()
    require_rounding(ref)
    if _ext.use_native(a):
        out = torch.ops.replicann.gemm_fp8_dgrad(qa, qb, sa, sb, a_bf8)
    else:
        deq = ops.dequantize_bf8 if a_bf8 else ops.dequantize_fp8
        out = (deq(qa, sa).float() @ ops.dequantize_fp8(qb, sb).float()).to(torch.bfloat16)
    assert_bitwise(out, expect_bf16(ref), what=f"gemm_fp8_dgrad a_bf8={a_bf8}")


def case_fp8_wgrad(device, M, N, K):
    """gemm_fp8_wgrad: dYᵀ·X with dY [K][M] e5m2, X [K][N] e4m3 (K = tokens): a bf16 output, an fp32
    output, accumulate into an fp32 output."""
    a, b, g = fp8_operands(device, M, N, K, 37 + M + N + K, deep_first=True)
    acc32 = int_operand((M, N), -1000, 1000, dtype=torch.float32, device=device, generator=g)
    (qa, sa), (qb, sb) = quant_e5m2(a), quant_e4m3(b)
    ref = a.double().t() @ b.double()
    require_rounding(ref)
    o16 = torch.full((M, N), SENTINEL, device=device, dtype=torch.bfloat16)
    o32 = torch.full((M, N), SENTINEL, device=device, dtype=torch.float32)
    oacc = acc32.clone()
    if _ext.use_native(a):
        torch.ops.replicann.gemm_fp8_wgrad(qa, qb, sa, sb, o16, False, True)
        torch.ops.replicann.gemm_fp8_wgrad(qa, qb, sa, sb, o32, False, True)
        torch.ops.replicann.gemm_fp8_wgrad(qa, qb, sa, sb, oacc, True, True)
    else:
        gf = ops.dequantize_bf8(qa, sa).float().t() @ ops.dequantize_fp8(qb, sb).float()
        o16.copy_(gf), o32.copy_(gf), oacc.add_(gf)
    miss = Misses()
    miss.check("bf16 out", o16, expect_bf16(ref))
    miss.check("fp32 out", o32, ref.float())
    miss.check("accumulate fp32", oacc, (acc32.double() + ref).float())
    miss.done()


# ------------------------------------------------------------------------------------------------
# group f: convolution as GEMM (representable class)
# ------------------------------------------------------------------------------------------------
def case_conv(device, C, OC, k, S, P, HW, batch=3, density=1.0):
    g = gen(23 + C + OC + HW)
    x = int_operand((batch, HW, HW, C), -1, 1, density=density, device=device, generator=g).requires_grad_()
    w = int_operand((OC, k, k, C), -1, 1, density=density, device=device, generator=g).requires_grad_()
    # the float64 reference (tiny) on the CPU
    x64 = x.detach().double().cpu().requires_grad_()
    w64 = w.detach().double().cpu().requires_grad_()
    y64 = F.conv2d(x64.permute(0, 3, 1, 2), w64.permute(0, 3, 1, 2), None, S, P).permute(0, 2, 3, 1)
    gy = int_operand(tuple(y64.shape), -1, 1, density=density, device=device, generator=g)
    y64.backward(gy.double().cpu())
    require_representable(y64.detach(), x64.grad, w64.grad)
    y = ops.conv2d_nhwc(x, w, None, S, P)
    y.backward(gy)
    miss = Misses()
    miss.check("y", y.detach(), expect_bf16(y64.detach()).to(device))
    miss.check("dx", x.grad, expect_bf16(x64.grad).to(device))
    miss.check("dw", w.grad, expect_bf16(w64.grad).to(device))
    miss.done()
