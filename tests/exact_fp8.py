"""Every byte and every state slot of the fp8 quantisers (csrc/kernels/fp8.hip) against the OCP formats.

bf16 -> e4m3 / e5m2 is exactly computable: every scale is a power of two, so x · (1 / scale) is exact in fp32, and
the product of two bf16 values (act_mul_bf8) is exact in fp32 too.  The expected byte of every element and the
expected bits of every state slot follow from the format alone, and the comparison is bitwise.

References, both on the CPU:
  encode     sign, clamp to ±max, round to nearest even, subnormals kept, in float64 / integer arithmetic, written
             from the OCP 8-bit floating point specification; never torch's float8 dtypes.
  decode     the table of the 256 values of a format, likewise.
  torch's float8 casts are the second implementation: tests/test_exact_fp8.py shows that the two agree on every
  finite bf16 value; the kernels are compared with ``encode``.
  pow2_ceil_ref / scale_ref: the kernel's documented scale rule (round up to a power of two, 1 for a non-positive
  input, the smallest normal for a subnormal quotient), the quotient hr · amax / max formed in fp32 as the kernel does.

Inputs are whole domains, not samples: ``value_table(fmt, k)`` is every finite bf16 value between a quarter of the
smallest subnormal and twice the maximum of the format at scale 2^k: every representable result, every midpoint
between two neighbours (a tie: bf16 has 4 - 5 more significand bits) with the bf16 neighbours on both sides, the
underflow tie, and values that saturate.  ``fill_index`` lays a table over n elements with a stride coprime to its
length, so the period lines up with neither a 16-byte chunk, a block nor a grid sweep; the expected bytes are the
same gather of the encoded table, which keeps the reference of a 16 M element case one vectorised pass.

Where the kernel evaluates GELU in fp32 (gelu_q8, act_mul_bf8(from_h=True)) the byte is not exactly computable: the
accepted bytes are the two encodings of the float64 value moved down and up by a derived evaluation bound, and the
test asserts that at most 1 % of the elements have more than one accepted byte (``case_gelu_q8``, ``case_act_mul_from_h``).

The cases run on any backend: ``Native`` (the raw ``torch.ops.replicann`` ops, tests/test_fp8_exact_gpu.py), ``Emu``
(a torch emulation built on the float8 casts; with a ``slip`` it is wrong in one way a kernel could be, and the CPU
tier asserts that the case fails) and ``OpsCpu`` (the CPU paths of replicann_amd.ops).  A plain module, not a conftest.
"""

import functools
import math
from typing import NamedTuple

import torch

from exact_ints import expect_bf16, gelu64, gelu_grad64, gen
from exact_rows import BF, U, Checks


# ------------------------------------------------------------------------------------------------
# the formats (OCP 8-bit floating point: e4m3 has no infinity and one NaN per sign, e5m2 is IEEE-like)
# ------------------------------------------------------------------------------------------------
class Fmt(NamedTuple):
    name: str
    ebits: int
    mbits: int
    bias: int
    max: float

    @property
    def emin(self):
        return 1 - self.bias

    @property
    def min(self):
        """The smallest subnormal."""
        return 2.0**(self.emin - self.mbits)

    @property
    def dtype(self):
        return torch.float8_e4m3fn if self.name == "e4m3" else torch.float8_e5m2

    @property
    def period(self):
        """The prime period of the position case (at most the number of finite codes)."""
        return 251 if self.name == "e4m3" else 241


E4M3 = Fmt("e4m3", 4, 3, 7, 448.0)
E5M2 = Fmt("e5m2", 5, 2, 15, 57344.0)

SWEEP = 2048 * 256  # chunks of 8 one sweep of the capped grid covers (fp8.hip gridn)
# n -> the branch it reaches in amax_k / quant_k / quant_delayed_k / quant_bf8_k / quant_delayed_bf8_k
SIZES = {1: "tail only", 7: "tail only", 8: "one chunk", 9: "chunk + tail", 2053: "a ragged last block + tail",
         8 * (SWEEP + 300) + 5: "a second grid-stride trip with a tail"}
N_BIG = 8 * (SWEEP + 300) + 5
# quant_delayed_bf8_k's 4-chunk loop: threads below 1000 take it once, all others the remainder loop three times
N_UNROLL = 8 * (3 * SWEEP + 1000) + 5
KS = (-20, 0, 10)
JUNK = (9.5, 8.25, 7.125, 6.0625)  # what a state slot holds before a call where the op must not read it

STATS = {}  # label -> dict(elements, mismatches, ambiguous): profiles/fp8_quantiser_parity.txt


def encode(v64, fmt, rounding="even", flush=False, bias_off=0, clamp=True):
    """The byte of every element of the float64 tensor ``v64`` (finite) in ``fmt``.

    |v| is clamped to the format's maximum; with e = max(floor(log2 |v|), emin) the spacing of the format around |v|
    is ulp = 2^(e - mbits), |v| / ulp is exact (a power of two) and k = its rounding to nearest, ties to even, lies
    in [0, 2^(mbits + 1)].  k < 2^mbits is a subnormal (exponent field 0, mantissa k); otherwise the code is
    (e - emin + 1) << mbits plus k - 2^mbits, which carries into the next exponent when k = 2^(mbits + 1).  A result
    that rounds to zero keeps its sign.  The keyword arguments are the deliberate mistakes of the CPU tier."""
    v = v64.double()
    if clamp:
        v = v.clamp(-fmt.max, fmt.max)
    neg, a = torch.signbit(v), v.abs()
    m, emin = fmt.mbits, fmt.emin - bias_off
    e = (torch.frexp(a)[1].long() - 1).clamp(min=emin)
    t = torch.ldexp(a, m - e)
    k = {"even": torch.round, "zero": torch.floor, "away": lambda z: torch.floor(z + 0.5)}[rounding](t).long()
    code = torch.where(k < (1 << m), k, ((e - emin + 1) << m) + (k - (1 << m)))
    if flush:
        code = torch.where(code < (1 << m), torch.zeros_like(code), code)
    if not clamp:  # beyond the range: the format's NaN (e4m3) or infinity (e5m2)
        code = torch.where(a > fmt.max, torch.full_like(code, 0x7F if fmt.name == "e4m3" else 0x7C), code)
    return ((code & 0x7F) | (neg.long() << 7)).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def decode_table(fmt):
    """float64 [256]: the value of every code."""
    b = torch.arange(256)
    e, f = (b >> fmt.mbits) & ((1 << fmt.ebits) - 1), (b & ((1 << fmt.mbits) - 1)).double()
    val = torch.where(e == 0, f * fmt.min, torch.ldexp(1 + f / (1 << fmt.mbits), e - fmt.bias))
    if fmt.name == "e4m3":
        val[(b & 0x7F) == 0x7F] = float("nan")
    else:
        top = e == (1 << fmt.ebits) - 1
        val[top & (f == 0)] = float("inf")
        val[top & (f != 0)] = float("nan")
    return torch.where(b >= 128, -val, val)


def finite_codes(fmt):
    return torch.isfinite(decode_table(fmt)).nonzero().flatten()


def pow2_ceil_ref(s):
    """fp8.hip pow2_ceil on the bits of the fp32 value ``s``, as a Python float."""
    s = torch.tensor(float(s), dtype=torch.float32)
    if not bool(s > 0):
        return 1.0
    u = int(s.view(torch.int32))
    e = u & 0x7F800000
    if e == 0x7F800000:
        return float(s)
    u = e + 0x00800000 if u & 0x007FFFFF else e
    return float(torch.tensor(u or 0x00800000, dtype=torch.int32).view(torch.float32))


def scale_ref(amax, fmt, hr=1.0):
    """The scale a quantiser derives from ``amax``: pow2_ceil(hr · amax / max), the quotient in fp32; 1 for 0."""
    a = torch.tensor(float(amax), dtype=torch.float32)
    if not bool(a > 0):
        return 1.0
    return pow2_ceil_ref((torch.tensor(hr, dtype=torch.float32) * a) / torch.tensor(fmt.max, dtype=torch.float32))


def log2i(s):
    m, e = math.frexp(s)
    assert m == 0.5, f"{s!r} is no power of two"
    return e - 1


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def finite_bf16():
    """Every finite bf16 value (65 280), in the order of the bit patterns."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]
    return bits.to(torch.int16).view(torch.bfloat16)


def bf16_next(v, up=True):
    """The bf16 neighbour of the positive bf16 value ``v`` (a float)."""
    b = torch.tensor(v, dtype=torch.bfloat16)
    assert float(b) == v and v > 0
    return float((b.view(torch.int16) + (1 if up else -1)).view(torch.bfloat16))


@functools.lru_cache(maxsize=8)
def value_table(fmt, k, below=None, at_most=None):
    """T(fmt, k): every finite bf16 v with min · 2^k / 4 <= |v| <= 2 · max · 2^k, and ±0; ``below`` / ``at_most``
    keep |v| < below / |v| <= at_most (the inputs of a current-scaling case stay under the planted amax)."""
    v = finite_bf16()
    a, s = v.double().abs(), 2.0**k
    keep = ((a >= fmt.min * s / 4) & (a <= 2 * fmt.max * s)) | (a == 0)
    if below is not None:
        keep &= a < below
    if at_most is not None:
        keep &= a <= at_most
    return v[keep]


def stride_for(L, base=389):
    a = base
    while math.gcd(a, L) != 1:
        a += 1
    return a


def fill_index(n, L, device, b=17):
    """(a · i + b) mod L with a coprime to L: consecutive elements differ, every table entry is reached."""
    return (torch.arange(n, device=device) * stride_for(L) + b) % L


def table_report(T, fmt, k):
    """What a table holds at scale 2^k: (results, ties, subnormal results, saturating values, underflow ties)."""
    v = T.double() / 2.0**k
    codes = encode(v, fmt)
    a = v.abs().clamp(max=fmt.max)
    t = torch.ldexp(a, fmt.mbits - (torch.frexp(a)[1].long() - 1).clamp(min=fmt.emin))
    ties = (t - torch.floor(t)) == 0.5  # (the two underflow ties included)
    return dict(codes=int(codes.unique().numel()), ties=int(ties.sum()),
                subnormal=int((((codes & 0x7F) < (1 << fmt.mbits)) & ((codes & 0x7F) > 0)).sum()),
                saturating=int((v.abs() > fmt.max).sum()), underflow_tie=int((v.abs() == fmt.min / 2).sum()))


# ------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------
def byte_report(q, exp, v64=None, fmt=None):
    """None, or the report of the bytes that differ: count, first and worst index, and (with the float64 quotient
    x / scale of every element) the count by class: tie, subnormal result, sign of a zero, saturation, other (which
    is what a byte in another element's place looks like)."""
    q, exp = q.reshape(-1), exp.reshape(-1).to(q.device)
    assert q.dtype == exp.dtype == torch.uint8 and q.shape == exp.shape, (q.dtype, exp.dtype, q.shape, exp.shape)
    bad = q != exp
    n = int(bad.sum())
    if n == 0:
        return None
    idx = bad.nonzero().flatten()
    first = int(idx[0])
    msg = (f"{n} of {q.numel()} bytes differ; first at {first}: got 0x{int(q[first]):02X}, expected "
           f"0x{int(exp[first]):02X}")
    if fmt is not None:
        dec = decode_table(fmt).to(q.device)
        d = (dec[q[idx].long()] - dec[exp[idx].long()]).abs()
        d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))
        w = int(idx[int(d.argmax())])
        msg += f"; worst at {w}: got 0x{int(q[w]):02X}, expected 0x{int(exp[w]):02X}"
        if v64 is not None:
            v = v64.reshape(-1).to(q.device)[idx].double()
            a, eb = v.abs(), exp[idx].long() & 0x7F
            ac = a.clamp(max=fmt.max)
            t = torch.ldexp(ac, fmt.mbits - (torch.frexp(ac)[1].long() - 1).clamp(min=fmt.emin))
            zero = (eb == 0) & ((q[idx].long() & 0x7F) == 0)
            tie = ~zero & ((t - torch.floor(t)) == 0.5)
            sat = ~zero & ~tie & (a > fmt.max)
            sub = ~zero & ~tie & ~sat & (eb < (1 << fmt.mbits))
            other = ~(zero | tie | sat | sub)
            msg += (f"; by class: tie {int(tie.sum())}, subnormal {int(sub.sum())}, sign of a zero {int(zero.sum())}, "
                    f"saturation {int(sat.sum())}, other (position) {int(other.sum())}")
            msg += f"; x / scale at the first: {float(v64.reshape(-1)[first])!r}"
    return msg


def f32_bits(t):
    return t.detach().float().cpu().view(torch.int32)


class Fp8Checks(Checks):
    """The misses of one case: bytes and state slots bitwise, plus the bounded checks of exact_rows.Checks."""

    def bytes(self, what, q, exp, v64=None, fmt=None):
        rep = byte_report(q, exp, v64, fmt)
        s = STATS.setdefault(self.label, dict(elements=0, mismatches=0, ambiguous=0))
        s["elements"] += q.numel()
        s["mismatches"] += int((q.reshape(-1) != exp.reshape(-1).to(q.device)).sum())
        if rep is not None:
            self.reports.append(f"[{what}] {rep}")

    def state(self, what, st, exp):
        """Every slot bit for bit (fp32)."""
        exp = torch.tensor([float(v) for v in exp], dtype=torch.float32)
        got = st.detach().float().cpu().reshape(-1)[:exp.numel()]
        bad = (f32_bits(got) != f32_bits(exp)).nonzero().flatten().tolist()
        if bad:
            self.reports.append(f"[{what}] state slots {bad} differ: got {[float(v).hex() for v in got]}, expected "
                                f"{[float(v).hex() for v in exp]}")


def junk_state(device, prev=None):
    st = torch.tensor(JUNK, device=device)
    if prev is not None:
        st[1] = prev
    return st


# ------------------------------------------------------------------------------------------------
# the ops under test
# ------------------------------------------------------------------------------------------------
class Native:
    """The raw ops."""

    def __getattr__(self, name):
        return getattr(torch.ops.replicann, name)

    def quant_many(self, flat, rows, states, max_n, qbuf, roll):
        segs = torch.tensor([[o, n, qo, states[i].data_ptr()] for i, (o, n, qo) in enumerate(rows)],
                            dtype=torch.int64).to(flat.device)
        torch.ops.replicann.fp8_quant_many(flat, segs, max_n, qbuf, roll)


ENC_SLIPS = {"round_toward_zero": dict(rounding="zero"), "ties_away": dict(rounding="away"),
             "flush_subnormal": dict(flush=True), "fnuz_bias": dict(bias_off=1)}
SLIPS = tuple(ENC_SLIPS) + ("no_clamp", "scale_round_down", "scale_not_pow2", "amax_skips_tail", "amax_first_sweep",
                             "words_swapped", "state2_not_written")

_GC = 0.7978845608028654
_L2E = 1.4426950408889634


def gelu_sig32(x):
    """common.h gelu_sig in torch fp32: 1 / (1 + exp2(x · (A · x² + B)))."""
    A = torch.tensor(-2.0 * _GC * 0.044715 * _L2E, dtype=torch.float32)
    B = torch.tensor(-2.0 * _GC * _L2E, dtype=torch.float32)
    return 1 / (1 + torch.exp2(x * (x * x * A + B)))


def gelu32(x):
    return x * gelu_sig32(x)


def gelu_grad32(x):
    s = gelu_sig32(x)
    k = x * (x * x * torch.tensor(2 * _GC * 0.134145, dtype=torch.float32) + torch.tensor(2 * _GC, dtype=torch.float32))
    return s * (k - s * k) + s


class Emu:
    """A torch emulation of the ops on CPU tensors, built on torch's float8 casts (the second implementation of the
    formats).  ``slip``: one deliberate mistake (SLIPS)."""

    def __init__(self, slip=None):
        assert slip is None or slip in SLIPS, slip
        self.slip = slip

    def _scale(self, amax, fmt, hr):
        amax = amax.float()
        if not bool(amax > 0):
            return torch.tensor(1.0)
        q = (torch.tensor(hr) * amax) / torch.tensor(fmt.max)
        if self.slip == "scale_not_pow2":
            return q
        m, e = torch.frexp(q)  # q = m · 2^e, m in [0.5, 1): up is 2^e (2^(e-1) for a power of two), down 2^(e-1)
        e = e - 1 if self.slip == "scale_round_down" else torch.where(m == 0.5, e - 1, e)
        return torch.ldexp(torch.tensor(1.0), e.clamp(min=-126)).float()

    def _amax(self, x, sweep=SWEEP):
        f = x.reshape(-1).float().abs()
        if self.slip == "amax_skips_tail":
            f = f[:f.numel() // 8 * 8]
        if self.slip == "amax_first_sweep":
            f = f[:sweep * 8]
        return f.max() if f.numel() else torch.tensor(0.0)

    def _bytes(self, x, scale, fmt):
        v = x.float() * (1 / scale.float())
        if self.slip in ENC_SLIPS:
            q = encode(v.double(), fmt, **ENC_SLIPS[self.slip])
        elif self.slip == "no_clamp":
            q = v.to(fmt.dtype).view(torch.uint8)
        else:
            q = v.clamp(-fmt.max, fmt.max).to(fmt.dtype).view(torch.uint8)
        if self.slip == "words_swapped":  # the two 32-bit words of every whole 8-byte chunk
            flat = q.reshape(-1)
            n8 = flat.numel() // 8 * 8
            flat[:n8] = flat[:n8].view(-1, 2, 4).flip(1).reshape(-1)
        return q

    def _roll(self, st, fmt):
        a = st[1].clone()
        if self.slip != "state2_not_written":
            st[2] = a
        st[0] = self._scale(a, fmt, 2.0)
        st[1] = 0

    def _delayed(self, x, st, fmt, sweep=SWEEP):
        q = self._bytes(x, st[0], fmt)
        st[1] = torch.maximum(st[1], self._amax(x, sweep))
        return q

    def _current(self, x, st, fmt):
        st[1] = self._amax(x)
        st[0] = self._scale(st[1], fmt, 1.0)
        return self._bytes(x, st[0], fmt)

    def fp8_quantize(self, x):
        st = torch.zeros(4)
        return self._current(x, st, E4M3), st

    def fp8_quantize_delayed(self, x, st):
        self._roll(st, E4M3)
        return self._delayed(x, st, E4M3)

    def bf8_quantize(self, x, st, delayed):
        if delayed:
            self._roll(st, E5M2)
            return self._delayed(x, st, E5M2)
        return self._current(x, st, E5M2)

    def quant_many(self, flat, rows, states, max_n, qbuf, roll):
        bx = min(max((max_n // 8 + 255) // 256, 1), 64)
        for i, (o, n, qo) in enumerate(rows):
            if roll:
                self._roll(states[i], E4M3)
            qbuf[qo:qo + n] = self._delayed(flat[o:o + n], states[i], E4M3, sweep=bx * 256)

    def fp8_dequantize(self, q, st):
        return (q.view(torch.float8_e4m3fn).float() * st[0]).to(torch.bfloat16)

    def bf8_dequantize(self, q, st):
        return (q.view(torch.float8_e5m2).float() * st[0]).to(torch.bfloat16)

    def act_mul_bf8(self, du, d, st, delayed, bias_grad=None, from_h=False):
        dh = du.float() * (gelu_grad32(d.float()) if from_h else d.float())
        if bias_grad is not None:
            bias_grad.copy_((bias_grad.float() + dh.sum(0)).to(torch.bfloat16))
        return self.bf8_quantize(dh, st, delayed)

    def gelu_q8(self, h, st):
        self._roll(st, E4M3)
        return self._delayed(gelu32(h.float()).to(torch.bfloat16), st, E4M3)


class OpsCpu:
    """The CPU paths of replicann_amd.ops (what a machine without the extension computes)."""

    def fp8_quantize(self, x):
        from replicann_amd import ops
        q, st = ops.quantize_fp8(x)
        q2, st2 = ops.Fp8State().quant(x, 0)  # the first quantisation of a slot is the same current scaling
        assert torch.equal(q, q2) and torch.equal(st, st2)
        return q, st

    def bf8_quantize(self, x, st, delayed):
        from replicann_amd import ops
        return ops.quantize_bf8(x, st, delayed)

    def fp8_dequantize(self, q, st):
        from replicann_amd import ops
        return ops.dequantize_fp8(q, st)

    def bf8_dequantize(self, q, st):
        from replicann_amd import ops
        return ops.dequantize_bf8(q, st)


def backend(device):
    return Native() if torch.device(device).type == "cuda" else Emu()


def _quant(be, fmt, x, st, delayed):
    """One single-tensor quantisation -> (bytes, state)."""
    if fmt is E4M3 and not delayed:
        return be.fp8_quantize(x)
    if fmt is E4M3:
        return be.fp8_quantize_delayed(x, st), st
    return be.bf8_quantize(x, st, delayed), st


# ------------------------------------------------------------------------------------------------
# 1. current scaling: fp8_quantize (amax_k + quant_k), bf8_quantize(delayed=False) (amax_k + quant_bf8_k)
# ------------------------------------------------------------------------------------------------
AMAX_CLASSES = ("exact", "above", "below")
PLANTS = ("first", "tail", "second")


def planted_amax(fmt, k, cls):
    """A: max · 2^k (the scale is 2^k and the top code is reached), one bf16 ulp above (the scale doubles), one below."""
    A = fmt.max * 2.0**k
    return A if cls == "exact" else bf16_next(A, cls == "above")


def plant_positions(n, plant):
    """Where ±A goes.  first: element 0.  tail: only among the n % 8 scalar-tail elements.  second: only in the
    second grid-stride trip (a chunk index of SWEEP + 100).  None where ``n`` has no such element."""
    if plant == "first":
        return [0]
    if plant == "tail":
        return [n - 1] if n % 8 and n > 8 else None
    return [8 * (SWEEP + 100) + 3] if n // 8 > SWEEP + 100 else None


def case_current(device, fmt, n, k, cls, plant, be=None):
    """Current scaling on T(fmt, k') below A, with -A planted (|.| is taken), k' the exponent of the expected scale.
    Expected: state [scale, amax, 0, 0] for e4m3 (the launcher clears all four floats); for e5m2 [scale, amax] and
    slots [2], [3] as they were (it clears two); bytes = encode(x / scale).  Returns False where ``n`` has no
    position for this plant."""
    be = be or backend(device)
    pos = plant_positions(n, plant)
    if pos is None:
        return False
    A = planted_amax(fmt, k, cls)
    scale = scale_ref(A, fmt)
    assert scale == 2.0**(k + (cls == "above")), (scale, k, cls)
    T = value_table(fmt, log2i(scale), below=A)
    idx = fill_index(n, T.numel(), device)
    x = T.to(device)[idx]
    exp = encode(T.double() / scale, fmt).to(device)[idx]
    x[pos] = -A
    exp[pos] = encode(torch.tensor([-A / scale], dtype=torch.float64), fmt).to(device)
    x0 = x.clone()
    st = junk_state(device)
    q, st = _quant(be, fmt, x, st, False)
    ck = Fp8Checks(f"current {fmt.name} n={n}")
    ck.bytes(f"k={k} A {cls} planted {plant}: bytes", q, exp, x0.double() / scale, fmt)
    ck.state(f"k={k} A {cls} planted {plant}: state", st,
             [scale, A, 0.0, 0.0] if fmt is E4M3 else [scale, A, *JUNK[2:]])
    ck.check_true("input", torch.equal(x, x0), "the input changed")
    ck.done()
    return True


def case_tiny(device, fmt=E4M3, n=2053, be=None):
    """amax = 2^-120: amax / max is subnormal in fp32, and the rule gives the smallest normal scale, 2^-126 (1 / scale
    = 2^126 is finite).  The inputs are every bf16 value below 2^-120 down to the smallest bf16 subnormal.  A
    quantiser whose division flushes the subnormal quotient takes pow2_ceil(0) = 1 and fails here."""
    be = be or backend(device)
    A = 2.0**-120
    scale = scale_ref(A, fmt)
    assert scale == 2.0**-126
    v = finite_bf16()
    T = v[v.double().abs() < A]
    idx = fill_index(n, T.numel(), device)
    x = T.to(device)[idx]
    exp = encode(T.double() * 2.0**126, fmt).to(device)[idx]
    x[n - 1], exp[n - 1] = A, encode(torch.tensor([64.0], dtype=torch.float64), fmt).to(device)
    q, st = _quant(be, fmt, x, junk_state(device), False)
    ck = Fp8Checks(f"tiny {fmt.name} n={n}")
    ck.bytes("bytes", q, exp, x.double() * 2.0**126, fmt)
    ck.state("state", st, [scale, A])
    ck.done()
    return float(st[0])


# ------------------------------------------------------------------------------------------------
# 2. delayed scaling: fp8_quantize_delayed (quant_delayed_k), bf8_quantize(delayed=True) (quant_delayed_bf8_k)
# ------------------------------------------------------------------------------------------------
def delayed_prev(fmt, kind):
    """prev: 0 (scale 1), max · 2^-13 (scale 2^-12: T(fmt, 0) saturates from |v| >= max · 2^-12 on), max · 2^11
    (scale 2^12: everything below min · 2^11 underflows)."""
    return {"zero": 0.0, "saturate": fmt.max * 2.0**-13, "underflow": fmt.max * 2.0**11}[kind]


PREVS = ("zero", "saturate", "underflow")


def case_delayed(device, fmt, n, prev_kind, be=None):
    """Two consecutive delayed quantisations on one state.  Before: [junk, prev, junk, junk].  Call 1 on T(fmt, 0):
    the scale is pow2_ceil(2 · prev / max) whatever x holds; after it [scale1, amax(x1), prev, junk].  Call 2 on
    T(fmt, k2), k2 the exponent of scale2 = pow2_ceil(2 · amax(x1) / max): [scale2, amax(x2), amax(x1), junk]."""
    be = be or backend(device)
    prev = delayed_prev(fmt, prev_kind)
    st = junk_state(device, prev)
    ck = Fp8Checks(f"delayed {fmt.name} n={n}")
    k = 0
    for call in (1, 2):
        scale = scale_ref(prev, fmt, 2.0)
        T = value_table(fmt, k)
        idx = fill_index(n, T.numel(), device, b=17 + call)
        x = T.to(device)[idx]
        exp = encode(T.double() / scale, fmt).to(device)[idx]
        q, st = _quant(be, fmt, x, st, True)
        amax = float(x.float().abs().max())
        ck.bytes(f"prev {prev_kind} call {call}: bytes", q, exp, x.double() / scale, fmt)
        ck.state(f"prev {prev_kind} call {call}: state", st, [scale, amax, prev, JUNK[3]])
        prev, k = amax, log2i(scale_ref(amax, fmt, 2.0))
    ck.done()


def case_position(device, fmt, n, delayed, be=None):
    """x[i] = s · decode(c[i mod P]), c the finite codes in order and P = 251 (e4m3) / 241 (e5m2), both prime and at
    most the number of finite codes (254 / 248: the NaN and infinity codes have no finite input).  The expected bytes
    are the code pattern itself, so two bytes or words swapped inside a chunk, or a chunk in another's place, show as
    a shifted index.  The top code is in the cycle, so current scaling finds the scale s as well."""
    be = be or backend(device)
    s = 2.0**-3
    codes = finite_codes(fmt)[:fmt.period]
    vals = (decode_table(fmt)[codes] * s)
    assert bool((vals.to(torch.bfloat16).double() == vals).all()) and float(vals.abs().max()) == fmt.max * s
    i = torch.arange(n, device=device) % fmt.period
    x = vals.to(torch.bfloat16).to(device)[i]
    exp = codes.to(torch.uint8).to(device)[i]
    prev = fmt.max * s / 2
    q, st = _quant(be, fmt, x, junk_state(device, prev), delayed)
    ck = Fp8Checks(f"position {fmt.name} n={n} delayed={int(delayed)}")
    ck.bytes("bytes", q, exp, x.double() / s, fmt)
    amax = float(x.float().abs().max())
    ck.state("state", st, [s, amax, prev] if delayed else [s, amax])
    ck.done()


# ------------------------------------------------------------------------------------------------
# 3. fp8_quant_many (fp8_roll_many_k + fp8_quant_many_k)
# ------------------------------------------------------------------------------------------------
MANY_SEGS = (5, 1000, 8 * 300, 300003)
SENT = 0xA5


def case_quant_many(device, roll, be=None):
    """Four segments of 5, 1000, 2400 and 300 003 elements in one flat buffer, laid out by the cache's rules (element
    offsets multiples of 64, byte offsets multiples of 16).  max_n = 300 003 gives the 64-block cap, which the
    largest segment needs three sweeps of, while the small ones see idle blocks.  roll: each slot goes
    [junk, prev, junk, junk] -> [pow2_ceil(2 · prev / 448), amax, prev, junk] as the single-tensor delayed op.
    roll = False: the scale already in slot [0] is used, the amax is folded into slot [1] by the same atomic max
    (so it ends as max(old, amax)), slots [2], [3] stay.  The bytes between and after the segments keep a sentinel;
    on the GPU the bytes and state of each segment must also equal fp8_quantize_delayed's."""
    be = be or backend(device)
    rows, off, qoff = [], 64, 16
    for n in MANY_SEGS:
        rows.append((off, n, qoff))
        off += (n + 63) // 64 * 64 + 64
        qoff += (n + 15) // 16 * 16 + 16
    g = gen(811)
    flat = torch.randn(off, generator=g).to(torch.bfloat16).to(device)
    qbuf = torch.full((qoff,), SENT, dtype=torch.uint8, device=device)
    prevs = [0.0, E4M3.max * 2.0**-5, E4M3.max * 2.0**3, E4M3.max * 2.0**-1]
    states = torch.tensor([JUNK] * 4, device=device)
    exp_q = torch.full((qoff,), SENT, dtype=torch.uint8)
    exp_st, singles = [], []
    for i, (o, n, qo) in enumerate(rows):
        scale = scale_ref(prevs[i], E4M3, 2.0)
        T = value_table(E4M3, log2i(scale))
        idx = fill_index(n, T.numel(), "cpu", b=5 + i)
        x = T[idx]
        flat[o:o + n] = x.to(device)
        exp_q[qo:qo + n] = encode(x.double() / scale, E4M3)
        amax = float(x.float().abs().max())
        if roll:
            states[i, 1] = prevs[i]
            exp_st.append([scale, amax, prevs[i], JUNK[3]])
        else:
            old = 0.0 if i % 2 == 0 else 4 * amax
            states[i, 0], states[i, 1] = scale, old
            exp_st.append([scale, max(old, amax), JUNK[2], JUNK[3]])
        if torch.device(device).type == "cuda":
            s1 = states[i].clone()
            if not roll:  # replay: the roll of the single-tensor op from the amax that gives this scale
                s1[1] = prevs[i]
            singles.append((be.fp8_quantize_delayed(flat[o:o + n].clone(), s1), s1))
    be.quant_many(flat, rows, states, max(MANY_SEGS), qbuf, roll)
    ck = Fp8Checks(f"quant_many roll={int(roll)}")
    ck.bytes("segments and the sentinel around them", qbuf, exp_q)
    for i, (o, n, qo) in enumerate(rows):
        ck.state(f"segment {i} ({n} elements): state", states[i], exp_st[i])
        if singles:
            ck.bytes(f"segment {i}: against fp8_quantize_delayed", qbuf[qo:qo + n], singles[i][0])
            if roll:
                ck.state(f"segment {i}: state against fp8_quantize_delayed", states[i], singles[i][1].tolist())
    ck.done()


# ------------------------------------------------------------------------------------------------
# 4. dequantise
# ------------------------------------------------------------------------------------------------
DEQ_SCALES = (2.0**-20, 1.0, 2.0**10, 0.3)
DEQ_N = (256, 256 * 9 + 3)


def case_dequant(device, fmt, n, scale, be=None):
    """All 256 codes, repeated to n, against bf16(fp32(decode(b)) · scale): decode(b) is exact in fp32, the product
    is one fp32 rounding (none for a power of two) and the store one bf16 rounding.  NaN and infinity codes are
    compared by class (and the sign of an infinity)."""
    be = be or backend(device)
    q = (torch.arange(n) % 256).to(torch.uint8)
    st = torch.tensor([scale, *JUNK[1:]], dtype=torch.float32)
    ref = (decode_table(fmt).float()[q.long()] * st[0]).to(torch.bfloat16)
    deq = be.fp8_dequantize if fmt is E4M3 else be.bf8_dequantize
    y = deq(q.to(device), st.to(device)).cpu()
    fin = torch.isfinite(ref.float())
    ck = Fp8Checks(f"dequant {fmt.name} n={n} scale={scale!r}")
    ck.check("finite codes", torch.where(fin, y, torch.zeros_like(y)).view(1, -1),
             torch.where(fin, ref, torch.zeros_like(ref)).view(1, -1))
    nan, inf = torch.isnan(ref.float()), torch.isinf(ref.float())
    ck.check_true("NaN codes", bool(torch.isnan(y.float())[nan].all()), "a NaN code did not decode to NaN")
    ck.check_true("infinity codes", bool((y.float()[inf] == ref.float()[inf]).all()),
                  "an infinity code decoded otherwise")
    ck.done()


# ------------------------------------------------------------------------------------------------
# 5. act_mul_bf8 (act_mul_bf8_k<MODE, FROM_H>), from_h = False: dH = dU ⊙ d is exact in fp32
# ------------------------------------------------------------------------------------------------
D_SET = (1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 0.75, 1.25)
ACT_MUL_SMALL = ((1, 8), (7, 24), (5, 1000))  # fewer threads than a block; dead threads inside block_max; G = M
ACT_MUL_LARGE = (5 * 2048 + 3, 1024)  # G = 2048: the 4-row loop once, the remainder loop once or twice


def act_mul_groups(M, N):
    """rn_act_mul_bf8_groups."""
    nc = N // 8
    return max(1, min((262144 + nc - 1) // nc, M))


def _d_index(i):
    return (3 * i + i // 8 + i // 1024) % len(D_SET)


def case_act_mul(device, M, N, k, delayed, be=None):
    """dU from T(e5m2, k) up to max · 2^(k - 1), d from {±1, ±0.5, ±2, 0.75, 1.25}: every product has at most 11
    significand bits, so dH is exact in fp32 (asserted); the products span the table at scale 2^k including its ties
    (d = ±1), the top code (max · 2^(k - 1) times -2, planted at element 0) and ties of their own (0.75, 1.25).
    Current scaling (MODE 0 then 1): state [scale, amax, untouched, untouched]; delayed (MODE 2) from
    prev = max · 2^(k - 1): [2^k, amax, prev, untouched].  Bytes, scale and amax bitwise."""
    be = be or backend(device)
    fmt, s = E5M2, 2.0**k
    T = value_table(fmt, k, at_most=fmt.max * s / 2)
    n = M * N
    i = torch.arange(n, device=device)
    ti, di = fill_index(n, T.numel(), device), _d_index(i)
    ti[0], di[0] = int((T.double() == fmt.max * s / 2).nonzero()[0]), D_SET.index(-2.0)
    dset = torch.tensor(D_SET, dtype=torch.bfloat16)
    P = T.double()[:, None] * dset.double()[None, :]
    assert bool(((T.float()[:, None] * dset.float()[None, :]).double() == P).all()), "precondition: dH exact in fp32"
    du, d = T.to(device)[ti].view(M, N), dset.to(device)[di].view(M, N)
    amax = fmt.max * s
    prev = amax / 2
    scale = scale_ref(prev, fmt, 2.0) if delayed else scale_ref(amax, fmt)
    assert scale == s
    exp = encode(P / scale, fmt).to(device)[ti, di]
    st = junk_state(device, prev)
    q = be.act_mul_bf8(du, d, st, delayed, None, False)
    ck = Fp8Checks(f"act_mul M={M} N={N} G={act_mul_groups(M, N)} delayed={int(delayed)}")
    ck.bytes(f"k={k}: bytes", q, exp, (P / scale).to(device)[ti, di], fmt)
    ck.state(f"k={k}: state", st, [scale, amax, prev if delayed else JUNK[2], JUNK[3]])
    ck.done()


def colsum_depth(M, G):
    """Roundings on the way of one column of the bias gradient: the rows one thread adds (act_mul_bf8_k's cs[]), then
    the column reduction of the G partial rows (common.h): G <= 1024: rn_colsum1_k, a chain of ceil(G / 16) per wave
    and a fold of 16; above: rn_colsum_k with 32 slabs, ceil(G / 128) per wave, a fold of 4 and a chain of 32; one
    more add into the old bias gradient."""
    per = -(-M // G)
    red = -(-G // 16) + 16 if G <= 1024 else -(-G // 128) + 4 + 32
    return per + red + 1


def case_act_mul_bias_grid(device, M, N, delayed, be=None):
    """bias_grad += Σ_rows dH with dU on a 2^-8 grid (N(0, 1/4), as exact_rows._grid) and d from D_SET: every dH is a
    multiple of 2^-10 and Σ_rows |dH| + |old| < 2^14 (asserted), so every partial sum in any order is exact in fp32
    and the result is the one bf16 rounding of old + Σ dH, with a non-zero old bias gradient."""
    be = be or backend(device)
    g = gen(907 + M + N)
    du = (0.5 * torch.randn(M, N, generator=g) / 2.0**-8).round().mul(2.0**-8).to(torch.bfloat16).to(device)
    d = torch.tensor(D_SET, dtype=torch.bfloat16).to(device)[_d_index(torch.arange(M * N, device=device))].view(M, N)
    old = (torch.randn(N, generator=g) / 2.0**-8).round().mul(2.0**-8).to(torch.bfloat16).to(device)
    dh = du.double() * d.double()
    assert float(dh.abs().sum(0).max() + old.double().abs().max()) < 2.0**14
    ref = old.double() + dh.sum(0)
    assert int((expect_bf16(ref).double() != ref).sum()) >= 0.1 * N or M < 4, "precondition: the sums round"
    bg = old.clone()
    st = junk_state(device, float(dh.abs().max()))
    be.act_mul_bf8(du, d, st, delayed, bg, False)
    ck = Fp8Checks(f"act_mul bias_grad grid M={M} N={N} delayed={int(delayed)}")
    ck.check("bias_grad", bg.view(1, -1), expect_bf16(ref).view(1, -1))
    ck.done()


def case_act_mul_bias_table(device, M, N, k=-8, be=None):
    """bias_grad on the table inputs of case_act_mul, per column against float64.  Every dH is exact, so the only
    errors are the fp32 additions: D = colsum_depth(M, G) of them on the way of a column, each at most u of a partial
    sum that is at most Σ|dH| + |old|, and the one bf16 rounding of the perturbed sum:
    |bg - (old + Σ dH)| <= 2^-8 · |old + Σ dH| + (1 + 2^-8) · D · u · (Σ_rows |dH| + |old|)."""
    be = be or backend(device)
    fmt, s = E5M2, 2.0**k
    T = value_table(fmt, k, at_most=fmt.max * s / 2)
    n = M * N
    ti, di = fill_index(n, T.numel(), device), _d_index(torch.arange(n, device=device))
    dset = torch.tensor(D_SET, dtype=torch.bfloat16)
    du, d = T.to(device)[ti].view(M, N), dset.to(device)[di].view(M, N)
    old = torch.randn(N, generator=gen(911)).to(torch.bfloat16).to(device)
    dh = du.double() * d.double()
    ref = old.double() + dh.sum(0)
    D = colsum_depth(M, act_mul_groups(M, N))
    bg = old.clone()
    be.act_mul_bf8(du, d, junk_state(device), False, bg, False)
    ck = Fp8Checks(f"act_mul bias_grad table M={M} N={N}")
    ck.bound("bias_grad", bg, ref, BF * ref.abs() + (1 + BF) * D * U * (dh.abs().sum(0) + old.double().abs()))
    ck.done()


# ------------------------------------------------------------------------------------------------
# 6. gelu_q8 and act_mul_bf8(from_h=True): bounded, with an ambiguity cap
# ------------------------------------------------------------------------------------------------
GELU_N = (8, 8 * 257, 8 * (8192 * 256 + 300))  # one chunk; a ragged second block; a second trip of the 8192-block grid
FROM_H = ((7, 24), (4099, 64))
H_MAX = 16.0
AMBIGUOUS_CAP = 0.01
GELU_PREV = 3.0  # scale 2^-6: gelu(h) >= 7 saturates, |gelu(h)| < 2^-16 underflows


@functools.lru_cache(maxsize=1)
def h_table():
    v = finite_bf16()
    return v[v.double().abs() <= H_MAX]


def sig_terms(h64):
    """(s, eps_s) for common.h gelu_sig at float64 h: s = 1 / (1 + e), e = 2^a, a = h · (A · h² + B).

    The fp32 evaluation, u = 2^-24: h² is exact (h is bf16).  The constants A and B are fp32 roundings (u each) and the
    fma rounds once, all terms of one sign: the factor carries 2u; the multiply by h one more: |Δa| <= 3u·|a|, which
    moves e by the factor 2^Δa: relative 3u·ln2·|a| <= 2.25u·|a|.  v_exp_f32 and v_rcp_f32 are accurate to 1 ulp,
    2u relative each; 1 + e rounds once (u).  A relative error δ of e moves s by δ · e / (1 + e) = δ · (1 - s):
    eps_s = ((2.25·|a| + 2)·(1 - s) + 3) · u.  The first term is what grows with the exp2 argument for negative h;
    for positive h the factor 1 - s removes it.  Where e overflows (a > 128, h < -10.1) the kernel's s is 0 (and
    subnormal, perhaps flushed, from a > 126 on); the true s < 2^-126 is then below every scale's half subnormal."""
    a = -2.0 * _GC * _L2E * h64 * (1 + 0.044715 * h64 * h64)
    s = torch.sigmoid(-a * math.log(2.0))
    one_minus = torch.sigmoid(a * math.log(2.0))
    return s, ((2.25 * a.abs() + 2) * one_minus + 3) * U


def gelu_accept(h64, scale, fmt=E4M3):
    """Per element: (lo byte, hi byte, |lo value|, |hi value|) of gelu_q8: g = h · s carries eps_s and the rounding
    of the product: eps = eps_s + u; the kernel rounds g to bf16, then quantises: the accepted bytes are
    encode(bf16(g · (1 ∓ eps)) / scale)."""
    s, eps_s = sig_terms(h64)
    g = h64 * s  # exact_ints.gelu64 is the same function, but 1 + tanh cancels for h << 0
    assert float((g - gelu64(h64)).abs().max()) < 1e-12
    eps = eps_s + U
    lo, hi = expect_bf16(g - g.abs() * eps).double(), expect_bf16(g + g.abs() * eps).double()
    return encode(lo / scale, fmt), encode(hi / scale, fmt), lo.abs(), hi.abs()


def case_gelu_q8(device, n, be=None):
    """gelu_q8 on every finite bf16 |h| <= 16 (33 538 values) laid over n elements: each byte must be one of the two
    accepted (gelu_accept; bound derived in sig_terms); the recorded amax lies between the maxima of the two
    candidates; the scale is pow2_ceil(2 · 3 / 448) = 2^-6 bitwise, [2] = 3, [3] untouched.  Asserted: at most 1 % of
    the elements have two accepted bytes.  Returns the ambiguous share."""
    be = be or backend(device)
    H = h_table()
    scale = scale_ref(GELU_PREV, E4M3, 2.0)
    lo, hi, alo, ahi = gelu_accept(H.double(), scale)
    idx = fill_index(n, H.numel(), device)
    h = H.to(device)[idx]
    st = junk_state(device, GELU_PREV)
    q = be.gelu_q8(h, st)
    return _accept_check(f"gelu_q8 n={n}", q, lo.to(device)[idx], hi.to(device)[idx], st,
                         [scale, None, GELU_PREV, JUNK[3]], float(torch.minimum(alo, ahi).to(device)[idx].max()),
                         float(torch.maximum(alo, ahi).to(device)[idx].max()))


def _accept_check(label, q, lo, hi, st, exp_state, amax_lo, amax_hi):
    ok = (q == lo) | (q == hi)
    amb = float((lo != hi).float().mean())
    ck = Fp8Checks(label)
    s = STATS.setdefault(label, dict(elements=0, mismatches=0, ambiguous=0))
    s["elements"] += q.numel()
    s["mismatches"] += int((~ok).sum())
    s["ambiguous"] = amb
    if not bool(ok.all()):
        bad = (~ok).reshape(-1).nonzero().flatten()
        f = int(bad[0])
        ck.reports.append(f"[bytes] {bad.numel()} of {q.numel()} bytes are neither accepted byte; first at {f}: got "
                          f"0x{int(q.reshape(-1)[f]):02X}, accepted 0x{int(lo.reshape(-1)[f]):02X} / "
                          f"0x{int(hi.reshape(-1)[f]):02X}")
    ck.check_true("ambiguity", amb <= AMBIGUOUS_CAP, f"{amb:.4%} of the elements have two accepted bytes (cap 1 %)")
    got = st.detach().float().cpu()
    ck.check_true("amax", amax_lo <= float(got[1]) <= amax_hi,
                  f"amax {float(got[1])!r} outside [{amax_lo!r}, {amax_hi!r}]")
    got = got.clone()
    got[1] = 0
    ck.state("state", got, [0.0 if v is None else v for v in exp_state])
    ck.done()
    return amb


def grad_terms(h64):
    """(d, Δd) for common.h gelu_grad_f: d = s + s·(k - s·k), k = h · (c1 · h² + c0).

    With P = s and Q = s·(1 - s)·k: s carries eps_s (sig_terms); k two rounded constants, an fma and a multiply: 3u;
    the inner fma k - s·k rounds once (u of |(1 - s)·k|) and sees the error of s times |k|: s·eps_s·|k|; the outer fma
    rounds once (u of |d|).  So |Δd| <= eps_s·|P| + (eps_s + 4u)·|Q| + eps_s·s²·|k| + u·|d|, an absolute bound: d crosses
    zero near h = -0.75 and no relative bound holds there."""
    s, eps_s = sig_terms(h64)
    k = 2 * _GC * h64 * (1 + 0.134145 * h64 * h64)
    Q = s * (1 - s) * k
    d = s + Q  # exact_ints.gelu_grad64 is the same function, but 1 + tanh cancels for h << 0
    assert float((d - gelu_grad64(h64)).abs().max()) < 1e-9
    return d, eps_s * s + (eps_s + 4 * U) * Q.abs() + eps_s * s * s * k.abs() + U * d.abs()


def case_act_mul_from_h(device, M, N, delayed, be=None):
    """act_mul_bf8(from_h=True): dH = dU · gelu'(h) in fp32, straight to e5m2.  h as in case_gelu_q8, dU from
    {±1, ±0.5, ±2, 0.75, 1.25} · 2^-7 (so the product adds one rounding, u, and no range of its own).  Accepted bytes:
    encode((dH ∓ Δ) / scale), Δ = |dU|·(Δd + u·|d|) (grad_terms), no bf16 step.  Delayed scaling from prev = 2^-7
    (scale pow2_ceil(2^-6 / 57344) = 2^-21, bitwise); current scaling takes its scale from the kernel's own amax,
    which must lie between the two candidates' maxima that give the same power of two (asserted on the reference).
    At most 1 % of the elements may have two accepted bytes."""
    be = be or backend(device)
    H = h_table()
    n = M * N
    hi_, di = fill_index(n, H.numel(), device), _d_index(torch.arange(n, device=device))
    dset = torch.tensor(D_SET, dtype=torch.bfloat16) * 2.0**-7
    d64, dd = grad_terms(H.double())
    P = d64[:, None] * dset.double()[None, :]
    Dl = dset.double().abs()[None, :] * (dd + U * d64.abs())[:, None]
    prev = 2.0**-7
    a_lo = float((P.abs() - Dl).clamp(min=0).to(device)[hi_, di].max())
    a_hi = float((P.abs() + Dl).to(device)[hi_, di].max())
    scale = scale_ref(prev, E5M2, 2.0) if delayed else scale_ref(a_lo, E5M2)
    assert delayed or scale == scale_ref(a_hi, E5M2), "precondition: both candidate maxima give one scale"
    lo, hi = encode((P - Dl) / scale, E5M2), encode((P + Dl) / scale, E5M2)
    # s < 2^-126 (h < -10): no normal fp32 holds it and the kernel's exp2 overflows from a > 128 on, so its s is a
    # subnormal or +0 and d = s·(1 + (1 - s)·k) may come out as +0 where the true d is a negative number far below
    # every subnormal of the format: both zero bytes are accepted there (the value is a zero either way, asserted)
    under = sig_terms(H.double())[0] < 2.0**-126
    assert bool((((lo | hi) & 0x7F)[under] == 0).all())
    lo[under], hi[under] = 0x00, 0x80
    h, du = H.to(device)[hi_].view(M, N), dset.to(device)[di].view(M, N)
    st = junk_state(device, prev)
    q = be.act_mul_bf8(du, h, st, delayed, None, True)
    return _accept_check(f"act_mul from_h M={M} N={N} delayed={int(delayed)}", q, lo.to(device)[hi_, di].view(M, N),
                         hi.to(device)[hi_, di].view(M, N), st,
                         [scale, None, prev if delayed else JUNK[2], JUNK[3]], a_lo, a_hi)


def clear_caches():
    for f in (value_table, finite_bf16, h_table):
        f.cache_clear()
