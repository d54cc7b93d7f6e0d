"""Attention-probability dropout checked against the mask the forward kernel itself used.

The kernels never store the dropout mask: the forward, the dQ pass and the dK/dV pass each regenerate it
from a counter hash of (seed, b, h, query, key), each with its own tiling and index expressions.  The
mask does not depend on V, so a forward with a one-hot probe V (V[key c0 + j] = e_j) returns the dropped,
rescaled, normalised probabilities Pd[b, h, q, c0 + j] themselves; ceil(Tk / D) such forwards return all
of Pd.  Its nonzero pattern is the keep mask M, which goes into a plain float64 autograd reference (and
into a bf16-rounding emulation of the kernels) for the real V and dO; the kernels' O, dQ, dK, dV at the
same seed are compared with those.  Nothing here reproduces the device hash, and nothing imports the
native extension: a backend is any object with

    forward(q, k, v, bias, scale, causal, p, seed) -> O
    forward_backward(q, k, v, go, bias, scale, causal, p, seed) -> (O, dQ, dK, dV)

in the (B, T, H, D) layout (bias: None or a float (1|B, Tq, Tk) tensor).  tests/test_attention_dropout_gpu.py
passes the HIP kernels, tests/test_attention_dropout_ref.py an emulation with deliberately wrong variants.
"""

import math
from dataclasses import dataclass

import torch

SEED = 123456789

# Check F: worst-row error of the kernels <= ROW_RATIO x the worst-row error of emulated_bf16, both against
# the same float64 reference with the same extracted mask.  Chosen as the smallest of {1.5, 2, 3} that clears
# the largest ratio measured on an MI355X by at least 25 %.  Measured over every case and tensor
# (profiles/attention_dropout_parity.txt): MFMA kernels, packed and host-seed paths 0.84 .. 1.06; generic
# kernels 0.51 .. 1.29 (D = 80 causal, dQ).  1.29 x 1.25 = 1.61 > 1.5, so R = 2.
ROW_RATIO = 2.0

VALUE_RTOL = 1.0e-2          # check D: two bf16 roundings (2^-8 each, 0.78 % together) + 28 %
FRO_TOL = {"O": 2e-2, "dQ": 4e-2, "dK": 4e-2, "dV": 4e-2}  # check E: the bounds of _attn_check
SIGMAS = 5.0                 # checks B and C
MIN_PAIRS = 1000             # check C: agreements over fewer pairs are not evaluated
TENSORS = ("O", "dQ", "dK", "dV")


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    H: int
    Tq: int
    Tk: int
    D: int
    causal: bool
    bias: str | None  # None | "randn" (1, Tq, Tk) | "tril" 0/1 (1, T, T) | "randn_inf" (B, Tq, Tk), -inf tail
    p: float
    seed: int = SEED
    data_seed: int = 0

    @property
    def scale(self):
        return 0.125 if self.D == 64 else 1 / math.sqrt(self.D)  # as _attn_check (tests/test_ops_gpu.py)


def mfma_cases(D):
    return [
        Case(f"c1_d{D}", 2, 3, 200, 200, D, True, None, 0.1),
        Case(f"c2_d{D}", 2, 3, 200, 200, D, False, None, 0.5),
        Case(f"c3_d{D}", 2, 2, 100, 260, D, True, None, 0.1),
        Case(f"c4_d{D}", 1, 2, 130, 70, D, False, "randn", 0.1),
        Case(f"c5_d{D}", 2, 2, 96, 96, D, False, "tril", 0.1),
        Case(f"c6_d{D}", 2, 2, 72, 72, D, True, "randn_inf", 0.1),
    ]


GENERIC_CASES = [
    Case("g1_d48", 2, 3, 40, 40, 48, True, None, 0.1),
    Case("g2_d48", 2, 3, 40, 40, 48, False, None, 0.1),
    Case("g3_d48", 2, 3, 40, 33, 48, False, "randn", 0.1),
    Case("g4_d80", 2, 3, 40, 40, 80, True, None, 0.1),
]
PACKED_CASE = Case("packed_d64", 2, 4, 200, 200, 64, True, None, 0.1)


def make_inputs(case, device="cpu"):
    """q, k, v, dO (randn, bf16) and the case's bias, drawn on the CPU from case.data_seed (the same values on
    every device)."""
    g = torch.Generator().manual_seed(1000 + case.data_seed)
    B, H, Tq, Tk, D = case.B, case.H, case.Tq, case.Tk, case.D
    q, go = (torch.randn(B, Tq, H, D, generator=g).to(torch.bfloat16).to(device) for _ in range(2))
    k, v = (torch.randn(B, Tk, H, D, generator=g).to(torch.bfloat16).to(device) for _ in range(2))
    bias = None
    if case.bias == "randn":
        bias = 0.5 * torch.randn(1, Tq, Tk, generator=g)
    elif case.bias == "tril":  # the reference decoder's 0/1 float mask, added
        bias = torch.tril(torch.ones(Tq, Tk)).unsqueeze(0)
    elif case.bias == "randn_inf":
        bias = 0.5 * torch.randn(B, Tq, Tk, generator=g)
        bias[1, :, Tk - 5:] = float("-inf")  # (causal rows still see key 0: no fully masked row)
    elif case.bias is not None:
        raise ValueError(case.bias)
    return q, k, v, go, (bias.to(device) if bias is not None else None)


# ------------------------------------------------------------------ the probe
def probe_dropped_probs(backend, q, k, bias, scale, causal, p, seed):
    """Pd (B, H, Tq, Tk) float32 as the backend's forward computed it: one forward per chunk of D keys with
    V[c0 + j] = e_j for the chunk's keys and zero elsewhere, so O[b, q, h, j] = Pd[b, h, q, c0 + j].  q, k,
    bias, seed, Tq and Tk are the same in every call (the mask index depends on them, not on V)."""
    B, Tq, H, D = q.shape
    Tk = k.shape[1]
    out = torch.zeros(B, H, Tq, Tk, dtype=torch.float32, device=q.device)
    for c0 in range(0, Tk, D):
        n = min(D, Tk - c0)
        j = torch.arange(n, device=q.device)
        v = torch.zeros(B, Tk, H, D, dtype=q.dtype, device=q.device)
        v[:, c0 + j, :, j] = 1
        o = backend.forward(q, k, v, bias, scale, causal, p, seed)
        out[..., c0:c0 + n] = o.float().permute(0, 2, 1, 3)[..., :n]
    return out


# ------------------------------------------------------------------ references
def _scores(q, k, scale, causal, bias, dtype):
    """(S, visible): S (B, H, Tq, Tk) with -inf outside the causal band; visible = in the band, finite bias."""
    s = q.transpose(1, 2).to(dtype) @ k.transpose(1, 2).to(dtype).transpose(-2, -1) * scale
    Tq, Tk = s.shape[-2:]
    if bias is not None:
        s = s + bias.to(dtype).unsqueeze(1)
    if causal:  # ops.attention_reference's form
        s = s.masked_fill(torch.ones(Tq, Tk, dtype=torch.bool, device=s.device).triu(1 + Tk - Tq), float("-inf"))
    return s, torch.isfinite(s)


def reference_fp64(q, k, v, go, M, p, scale, causal, bias):
    """Plain float64 autograd: P = softmax(S), Pd = P·M/(1-p), O = Pd·V.  Returns (O, dQ, dK, dV, Pd)."""
    qd, kd, vd = (t.detach().double().requires_grad_() for t in (q, k, v))
    s, _ = _scores(qd, kd, scale, causal, bias, torch.float64)
    pd = torch.softmax(s, dim=-1) * M.double() / (1.0 - p)
    o = (pd @ vd.transpose(1, 2)).transpose(1, 2)
    o.backward(go.double())
    return o.detach(), qd.grad, kd.grad, vd.grad, pd.detach()


def _r(x):
    return x.to(torch.bfloat16).float()


def emulate_passes(q, k, v, go, masks, p, scale, causal, bias, rd=None, l_dropped=False):
    """The three kernels in fp32 torch with their roundings, each pass with its own mask and its own
    1/(1-p) factor — masks = (forward, dQ, dK/dV), rd likewise — so that tests can build passes that
    disagree.  Forward: the unnormalised P·M·rd is rounded to bf16 before P·V, the row sum l is taken over
    the undropped fp32 P (l_dropped: over the dropped P, a deliberate error), O = (P·V)/l is rounded to bf16.
    Backward: P = exp(S - lse) in fp32, δ = rowsum(dO ∘ O) from the bf16 O, dP = dO·Vᵀ; the dQ pass rounds
    dS = P·(dP·M·rd − δ) to bf16 before dS·K, the dK/dV pass rounds P·M·rd and its dS to bf16 before Pᵀ·dO and
    dSᵀ·Q; gradients are rounded to bf16.  go = None: forward only.  Returns (O, dQ, dK, dV) as float32."""
    mf, mq, mkv = (m.float() for m in masks)
    keep = 1.0 / (1.0 - p)
    rf, rq, rkv = rd if rd is not None else (keep, keep, keep)
    s, _ = _scores(q, k, scale, causal, bias, torch.float32)
    qt, kt, vt = (t.transpose(1, 2).float() for t in (q, k, v))
    mx = s.amax(-1, keepdim=True)
    pu = torch.exp(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))
    pdu = pu * mf * rf
    l = (pdu if l_dropped else pu).sum(-1, keepdim=True)
    inv = torch.where(l > 0, 1 / l, torch.zeros_like(l))
    o = _r((_r(pdu) @ vt) * inv)
    if go is None:
        return o.transpose(1, 2), None, None, None
    gt = go.transpose(1, 2).float()
    pn = pu * inv
    delta = (gt * o).sum(-1, keepdim=True)
    dp = gt @ vt.transpose(-2, -1)
    dq = _r(_r(pn * (dp * mq * rq - delta)) @ kt * scale)
    dv = _r(_r(pn * mkv * rkv).transpose(-2, -1) @ gt)
    dk = _r(_r(pn * (dp * mkv * rkv - delta)).transpose(-2, -1) @ qt * scale)
    return tuple(t.transpose(1, 2) for t in (o, dq, dk, dv))


def emulated_bf16(q, k, v, go, M, p, scale, causal, bias):
    """The operation with mask M in fp32 and the kernels' bf16 roundings (see emulate_passes): what a correct
    kernel's rounding error looks like.  A reference: it calls nothing from the native extension."""
    return emulate_passes(q, k, v, go, (M, M, M), p, scale, causal, bias)


# ------------------------------------------------------------------ norms
def rel_fro(a, ref):
    """The suite's whole-tensor norm (rel_err in tests/test_ops_gpu.py)."""
    a, ref = a.double(), ref.double()
    return ((a - ref).norm() / (ref.norm() + 1e-12)).item()


def row_err(a, ref):
    """max over the length-D rows of ‖a_row − ref_row‖ / max(‖ref_row‖, rms over rows of ‖ref_row‖): an error
    confined to a few rows shows here at full size; the rms floor keeps near-zero rows from dominating."""
    a, ref = a.double().reshape(-1, a.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    rn = ref.norm(dim=-1)
    floor = rn.pow(2).mean().sqrt()
    return ((a - ref).norm(dim=-1) / torch.maximum(rn, floor)).max().item()


# ------------------------------------------------------------------ the checks
class CheckFailure(AssertionError):
    """Raised by check_case after all checks ran: .failed lists (check, tensor or quantity) of every failed
    check in order A..F, .measured holds every measured value."""

    def __init__(self, failed, messages, measured):
        super().__init__("\n".join(messages))
        self.failed, self.measured = failed, measured


def _agreement(ma, mb, valid):
    n = int(valid.sum().item())
    return (((ma == mb) & valid).sum().item() / n if n else float("nan")), n


def mask_structure(M, vis, p, shifts):
    """Check C's measurements on a boolean mask: {name: (agreement, pairs, deviation in σ)} of M with itself
    shifted along the given (dim, shift) pairs, between heads 0 / 1 and batches 0 / 1 where present; entries
    with fewer than MIN_PAIRS pairs are left out.  Independent Bernoulli(1-p) entries agree with probability
    a = (1-p)² + p², σ = sqrt(a(1-a)/n)."""
    a = (1 - p) ** 2 + p ** 2
    out = {}

    def put(name, ma, mb, valid):
        ag, n = _agreement(ma, mb, valid)
        if n >= MIN_PAIRS:
            out[name] = (ag, n, abs(ag - a) / math.sqrt(a * (1 - a) / n))

    for name, dim, s in shifts:
        if s < M.shape[dim]:
            lo, hi = M.narrow(dim, 0, M.shape[dim] - s), M.narrow(dim, s, M.shape[dim] - s)
            put(name, lo, hi, vis.narrow(dim, 0, M.shape[dim] - s) & vis.narrow(dim, s, M.shape[dim] - s))
    if M.dim() == 4:
        if M.shape[1] > 1:
            put("head0_vs_head1", M[:, 0], M[:, 1], vis[:, 0] & vis[:, 1])
        if M.shape[0] > 1:
            put("batch0_vs_batch1", M[0], M[1], vis[0] & vis[1])
    return out


ATTN_SHIFTS = [(f"key+{s}", 3, s) for s in (1, 16, 32, 64)] + [(f"query+{s}", 2, s) for s in (1, 16, 64)]


def keep_rate(M, vis, p):
    """Check B's measurements: (mean of M over the visible entries, their number N, deviation from 1-p in σ)."""
    n = int(vis.sum().item())
    rate = (M & vis).sum().item() / n
    return rate, n, abs(rate - (1 - p)) / math.sqrt(p * (1 - p) / n)


def check_case(backend, case, device="cpu", row_ratio=None):
    """Checks A to F (see the module docstring and the comments below) of `backend` on `case`.  Every check is
    evaluated and recorded with its measured value; if any failed, CheckFailure lists them all.  Returns the
    measured values."""
    R = ROW_RATIO if row_ratio is None else row_ratio
    q, k, v, go, bias = make_inputs(case, device)
    p, scale, causal = case.p, case.scale, case.causal
    failed, msgs, m = [], [], {"case": case.name}

    def check(ok, name, what, text):
        if not ok:
            failed.append((name, what))
            msgs.append(f"{case.name} check {name} [{what}]: {text}")

    probe = probe_dropped_probs(backend, q, k, bias, scale, causal, p, case.seed)
    _, vis = _scores(q, k, scale, causal, bias, torch.float64)
    vis = vis.expand(probe.shape)
    M = (probe != 0) & vis

    # A. support: the mask is the probe's nonzero pattern on visible entries (finite, non-negative values);
    #    outside the causal band and at -inf bias the probe is exactly 0
    bad = int((~torch.isfinite(probe) | (probe < 0)).sum().item())
    check(bad == 0, "A", "finite", f"{bad} probed values are negative or not finite")
    leak = int(((probe != 0) & ~vis).sum().item())
    m["A_invisible_nonzero"] = leak
    check(leak == 0, "A", "invisible", f"{leak} invisible entries of the probe are not 0")

    # B. keep rate over the N visible entries
    rate, n, dev = keep_rate(M, vis, p)
    m["B_keep_rate"], m["B_n"], m["B_sigma"] = rate, n, dev
    check(dev <= SIGMAS, "B", "keep rate", f"mean(M) = {rate:.5f} over {n} entries, {dev:.2f}σ from {1 - p}")

    # C. no structure in the mask; the same seed reproduces it bitwise, another seed is independent of it
    m["C"] = mask_structure(M, vis, p, ATTN_SHIFTS)
    for name, (ag, npairs, d) in m["C"].items():
        check(d <= SIGMAS, "C", name, f"agreement {ag:.5f} over {npairs} pairs, {d:.2f}σ from (1-p)²+p²")
    again = probe_dropped_probs(backend, q, k, bias, scale, causal, p, case.seed)
    m["C_same_seed_bitwise"] = bool(torch.equal(again, probe))
    check(m["C_same_seed_bitwise"], "C", "same seed", "the same seed gave a different probe")
    other = probe_dropped_probs(backend, q, k, bias, scale, causal, p, case.seed + 1)
    a = (1 - p) ** 2 + p ** 2
    ag, npairs = _agreement(M, (other != 0) & vis, vis)
    d = abs(ag - a) / math.sqrt(a * (1 - a) / npairs)
    m["C_other_seed"] = (ag, npairs, d)
    check(d <= SIGMAS, "C", "other seed", f"agreement {ag:.5f} with seed+1 over {npairs} entries, {d:.2f}σ from {a:.4f}")

    # D. values: every kept element against softmax(S)·M/(1-p) in float64
    ref_o, ref_dq, ref_dk, ref_dv, pd_ref = reference_fp64(q, k, v, go, M, p, scale, causal, bias)
    rel = ((probe.double() - pd_ref).abs() / pd_ref.clamp_min(1e-300))[M]
    m["D_max_rel"] = rel.max().item() if rel.numel() else 0.0
    check(m["D_max_rel"] <= VALUE_RTOL, "D", "probe values",
          f"max |probe - Pd_ref| / Pd_ref = {m['D_max_rel']:.3e} > {VALUE_RTOL:.1e}")

    # E. whole tensor, F. worst row: the kernels and the emulation against the same float64 reference and mask
    refs = dict(zip(TENSORS, (ref_o, ref_dq, ref_dk, ref_dv)))
    got = dict(zip(TENSORS, backend.forward_backward(q, k, v, go, bias, scale, causal, p, case.seed)))
    emu = dict(zip(TENSORS, emulated_bf16(q, k, v, go, M, p, scale, causal, bias)))
    for t in TENSORS:
        fro = rel_fro(got[t], refs[t])
        m[f"E_fro_{t}"] = fro
        check(fro < FRO_TOL[t], "E", t, f"rel_fro = {fro:.3e}, bound {FRO_TOL[t]:.0e}")
    for t in TENSORS:
        rk, re = row_err(got[t], refs[t]), row_err(emu[t], refs[t])
        m[f"F_row_{t}"], m[f"F_row_emu_{t}"], m[f"F_ratio_{t}"] = rk, re, rk / re
        m[f"E_fro_emu_{t}"] = rel_fro(emu[t], refs[t])
        check(rk <= R * re, "F", t, f"row_err = {rk:.3e} = {rk / re:.2f} x the emulation's {re:.3e}, bound {R} x")
    if failed:
        raise CheckFailure(failed, msgs, m)
    return m
