"""CPU tier of the fp8 quantiser checks (tests/exact_fp8.py).

The references check each other: the integer encoder against torch's float8 casts on every finite bf16 value, the
decode table against the encoder.  The scale rule's edges (replicann_amd.ops.fp8.pow2_ceil against the kernel's rule).
Every case of tests/test_fp8_exact_gpu.py at its small sizes on the emulation and on the CPU paths of
replicann_amd.ops.  And the reason for bitwise checks: each case is run against an emulation that is wrong in one
way a quantiser could be (exact_fp8.SLIPS) and must fail, while ``old_assertions`` says which of the suite's earlier
tolerances (99 % / 99.9 % of the bytes, a 5 % / 10 % norm, amax to 1e-3) let the same mistake through."""

import exact_fp8 as X
import pytest
import torch

from replicann_amd.ops.fp8 import _pow2_ceil_pos, pow2_ceil

CPU = torch.device("cpu")
FMTS = [X.E4M3, X.E5M2]
SMALL = [n for n in X.SIZES if n < 10000]


@pytest.fixture(scope="module", autouse=True)
def _drop_tables():
    yield
    X.clear_caches()


# ---- the references -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.name)
def test_encoder_agrees_with_torch_cast_on_every_finite_bf16(fmt):
    x = X.finite_bf16()
    assert x.numel() == 65280
    for k in X.KS:
        mine = X.encode(x.double() / 2.0**k, fmt)
        ref = (x.float() / 2.0**k).clamp(-fmt.max, fmt.max).to(fmt.dtype).view(torch.uint8)
        assert X.byte_report(mine, ref, x.double() / 2.0**k, fmt) is None
        assert mine.unique().numel() == (254 if fmt is X.E4M3 else 248)  # every finite code: no NaN, no infinity


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.name)
def test_decode_table_inverts_the_encoder(fmt):
    dec = X.decode_table(fmt)
    codes = X.finite_codes(fmt)
    assert codes.numel() == (254 if fmt is X.E4M3 else 248)
    assert torch.equal(X.encode(dec[codes], fmt).long(), codes)
    assert torch.equal(dec[codes].float(), codes.to(torch.uint8).view(fmt.dtype).float())  # torch's own table
    assert float(dec[codes].max()) == fmt.max and float(dec[1]) == fmt.min
    sat = X.encode(torch.tensor([3 * fmt.max, -3 * fmt.max], dtype=torch.float64), fmt).tolist()
    assert sat == ([0x7E, 0xFE] if fmt is X.E4M3 else [0x7B, 0xFB])
    # the underflow tie goes to zero (even), its upper bf16 neighbour to the smallest subnormal; a zero keeps its sign
    t = torch.tensor([fmt.min / 2, X.bf16_next(fmt.min / 2), -fmt.min / 2, -0.0], dtype=torch.float64)
    assert X.encode(t, fmt).tolist() == [0x00, 0x01, 0x80, 0x80]


def test_pow2_ceil_follows_the_kernel_rule():
    ordinary = [0.0, -1.0, 1.0, 0.75, 1.5, 2.0, 3.0, 2 * 3.0 / 448, 2.0**-20, 1.0000001, 0.99999994, 2.0**100 * 1.5]
    for s in ordinary:
        assert pow2_ceil(s).item() == X.pow2_ceil_ref(s), s
    # amax / 448 at the edge of the normal range: subnormal, exactly the smallest normal, just above it
    for amax, want in ((2.0**-120, 2.0**-126), (448 * 2.0**-126, 2.0**-126), (449 * 2.0**-126, 2.0**-125)):
        q = torch.tensor(amax, dtype=torch.float32) / 448
        assert pow2_ceil(q).item() == want == X.pow2_ceil_ref(q) == X.scale_ref(amax, X.E4M3)
        assert torch.isfinite(1 / pow2_ceil(q))
    t = torch.tensor([0.0, 0.75, 1.0, 2.0**-130, 2.0**-149, 3.0])
    assert _pow2_ceil_pos(t).tolist() == [0.0, 1.0, 1.0, 2.0**-126, 2.0**-126, 4.0]


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.name)
def test_value_table_holds_the_whole_domain(fmt):
    for k in X.KS:
        T = X.value_table(fmt, k)
        rep = X.table_report(T, fmt, k)
        assert 5000 < T.numel() < 10000 and T.numel() == T.unique().numel() + 1  # ±0 are one value to unique()
        assert rep["codes"] == (254 if fmt is X.E4M3 else 248)
        assert rep["ties"] == rep["codes"] - 2 and rep["underflow_tie"] == 2  # every gap between neighbours, 0 included
        assert rep["subnormal"] > 0 and rep["saturating"] >= 2 * 100
        # the bf16 neighbours on both sides of the underflow tie are there
        a = T.double().abs() / 2.0**k
        assert bool((a == X.bf16_next(fmt.min / 2)).any()) and bool((a == X.bf16_next(fmt.min / 2, False)).any())
    idx = X.fill_index(3 * T.numel(), T.numel(), CPU)
    assert idx[:T.numel()].unique().numel() == T.numel() and bool((idx[1:] != idx[:-1]).all())


# ---- the cases on the emulation, and on the CPU paths of the package ------------------------------
@pytest.mark.parametrize("be", [X.Emu, X.OpsCpu], ids=["emu", "ops"])
@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.name)
def test_current_scaling(fmt, be):
    ran = 0
    for n in SMALL:
        for k in X.KS:
            for cls in X.AMAX_CLASSES:
                for plant in X.PLANTS:
                    ran += X.case_current(CPU, fmt, n, k, cls, plant, be=be())
    assert ran == 9 * (len(SMALL) + 2)  # planted first at every size, in the tail at n = 9 and 2053
    assert X.case_tiny(CPU, fmt, be=be()) == 2.0**-126


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.name)
def test_delayed_scaling(fmt):
    for n in SMALL:
        for prev in X.PREVS:
            X.case_delayed(CPU, fmt, n, prev)


def test_delayed_scaling_e5m2_on_the_cpu_path():
    for n in SMALL:
        for prev in X.PREVS:
            X.case_delayed(CPU, X.E5M2, n, prev, be=X.OpsCpu())


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.name)
def test_position(fmt):
    for delayed in (False, True):
        X.case_position(CPU, fmt, 2053, delayed)
    X.case_position(CPU, fmt, 2053, False, be=X.OpsCpu())


@pytest.mark.parametrize("roll", [True, False])
def test_quant_many(roll):
    X.case_quant_many(CPU, roll)


@pytest.mark.parametrize("be", [X.Emu, X.OpsCpu], ids=["emu", "ops"])
@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f.name)
def test_dequantise(fmt, be):
    for n in X.DEQ_N:
        for scale in X.DEQ_SCALES:
            X.case_dequant(CPU, fmt, n, scale, be=be())


@pytest.mark.parametrize("delayed", [False, True])
def test_act_mul(delayed):
    for M, N in X.ACT_MUL_SMALL:
        for k in X.KS:
            X.case_act_mul(CPU, M, N, k, delayed)
        X.case_act_mul_bias_grid(CPU, M, N, delayed)
        X.case_act_mul_bias_table(CPU, M, N)


def test_gelu_q8_and_from_h_stay_under_the_ambiguity_cap():
    for n in X.GELU_N[:2]:
        assert X.case_gelu_q8(CPU, n) <= X.AMBIGUOUS_CAP
    # the whole h table once: the share of the domain itself
    assert X.case_gelu_q8(CPU, 8 * (X.h_table().numel() // 8 + 1)) <= X.AMBIGUOUS_CAP
    for M, N in X.FROM_H:
        for delayed in (False, True):
            assert X.case_act_mul_from_h(CPU, M, N, delayed) <= X.AMBIGUOUS_CAP


# ---- each check bites ---------------------------------------------------------------------------
def old_assertions(slip):
    """Which of the earlier tolerances the mistake passes, on the earlier tests' kind of input (79 200 normal samples
    at one scale): e4m3 bytes > 99 % equal to the cast; e5m2 bytes < 0.1 % different; dequantised rel_err < 0.05;
    the delayed pass's norm < 0.1; the recorded amax to 1e-3 relative."""
    x = (3 * torch.randn(300, 264, generator=X.gen(20))).to(torch.bfloat16)
    be = X.Emu(slip)
    q, st = be.fp8_quantize(x)
    ref = (x.float() / st[0]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    deq = X.Emu().fp8_dequantize(q, st).double()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    s5 = torch.zeros(4)
    q5 = be.bf8_quantize(x, s5, False)
    ref5 = (x.float() / s5[0]).to(torch.float8_e5m2).view(torch.uint8)
    q5d = be.bf8_quantize(x * 0.5, s5, True)
    deq5 = X.Emu().bf8_dequantize(q5d, s5).double()
    amax = float(x.float().abs().max())
    return dict(bytes_99=float((q == ref).float().mean()) > 0.99, bytes_999=float((q5 != ref5).float().mean()) < 1e-3,
                rel_005=rel(deq, x.double()) < 0.05, norm_01=rel(deq5, 0.5 * x.double()) < 0.1,
                amax_1e3=abs(float(st[1]) - amax) < 1e-3 * amax and abs(float(s5[1]) - 0.5 * amax) < 1e-3 * amax)


# slip -> (the case that must fail, what its report must name, the earlier assertions that pass the mistake)
MUTANTS = {
    "round_toward_zero": (lambda be: X.case_delayed(CPU, X.E4M3, 2053, "zero", be=be), r"by class: tie \d+",
                          {"rel_005", "norm_01", "amax_1e3"}),
    "ties_away": (lambda be: X.case_delayed(CPU, X.E5M2, 2053, "zero", be=be), r"by class: tie \d+, subnormal 0, ",
                  {"rel_005", "norm_01", "amax_1e3"}),
    "flush_subnormal": (lambda be: X.case_delayed(CPU, X.E4M3, 2053, "zero", be=be), r"subnormal [1-9]\d*",
                        {"bytes_99", "bytes_999", "rel_005", "norm_01", "amax_1e3"}),
    "fnuz_bias": (lambda be: X.case_delayed(CPU, X.E4M3, 2053, "zero", be=be), r"bytes differ", {"amax_1e3"}),
    "no_clamp": (lambda be: X.case_delayed(CPU, X.E5M2, 2053, "saturate", be=be), r"saturation [1-9]\d*",
                 {"bytes_99", "bytes_999", "rel_005", "norm_01", "amax_1e3"}),
    "scale_round_down": (lambda be: X.case_current(CPU, X.E4M3, 2053, 0, "below", "first", be=be), r"state slots \[0\]",
                         {"bytes_99", "norm_01", "amax_1e3"}),
    "scale_not_pow2": (lambda be: X.case_current(CPU, X.E5M2, 2053, -20, "below", "first", be=be), r"state slots \[0\]",
                       {"bytes_99", "rel_005", "norm_01", "amax_1e3"}),
    "amax_skips_tail": (lambda be: X.case_current(CPU, X.E4M3, 9, 10, "exact", "tail", be=be), r"state slots \[0, 1\]",
                        {"bytes_99", "bytes_999", "rel_005", "norm_01", "amax_1e3"}),
    "amax_first_sweep": (lambda be: X.case_current(CPU, X.E5M2, X.N_BIG, 0, "exact", "second", be=be),
                         r"state slots \[1\]", {"bytes_99", "bytes_999", "rel_005", "norm_01", "amax_1e3"}),
    "words_swapped": (lambda be: X.case_position(CPU, X.E4M3, 2053, True, be=be), r"other \(position\) [1-9]\d*",
                      {"amax_1e3"}),
    "state2_not_written": (lambda be: X.case_delayed(CPU, X.E4M3, 9, "saturate", be=be), r"state slots \[2\]",
                           {"bytes_99", "bytes_999", "rel_005", "norm_01", "amax_1e3"}),
}


def test_every_slip_has_a_case():
    assert set(MUTANTS) == set(X.SLIPS)


@pytest.mark.parametrize("slip", X.SLIPS)
def test_slip_fails_its_case(slip):
    run, match, old_pass = MUTANTS[slip]
    with pytest.raises(AssertionError, match=match):
        run(X.Emu(slip))
    run(X.Emu())  # and the case passes without the mistake
    got = {k for k, v in old_assertions(slip).items() if v}
    assert got == old_pass, (slip, sorted(got))
