"""The attention-dropout checker (tests/attn_dropout_ref.py) tested on the CPU with an emulated backend:
emulate_passes (the kernels' math and roundings in torch) plus a counter-based torch mask.  The correct
backend passes every check; each deliberately wrong backend — the slips the GPU tests exist to catch — fails
at the check named for it.  This is the evidence, on a machine without a GPU, that
tests/test_attention_dropout_gpu.py would notice a subtly wrong kernel."""

import pytest
import torch

import attn_dropout_ref as adr

_M64 = (1 << 64) - 1


def _i64(c):
    return c - (1 << 64) if c >= (1 << 63) else c


def _lsr(x, s):
    return (x >> s) & ((1 << (64 - s)) - 1)


def counter_mask(seed, B, H, Tq, Tk, p, device, per_head=True, key_period=None):
    """Keep mask (B, H, Tq, Tk) from a splitmix64-style hash of (seed, element index) in wrapping int64
    arithmetic (any counter-based mask serves; it is not the device hash).  per_head=False drops the head
    from the index, key_period folds the key index: the two structured masks check C must reject."""
    b, h, qi, kj = torch.meshgrid(*(torch.arange(n, device=device) for n in (B, H, Tq, Tk)), indexing="ij")
    if not per_head:
        h = torch.zeros_like(h)
    if key_period:
        kj = kj % key_period
    z = ((b * H + h) * Tq + qi) * Tk + kj + _i64((seed * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & _M64)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    return _lsr(z, 40).double() / float(1 << 24) >= p


class EmuBackend:
    """emulate_passes behind the backend interface.  dq_mask / dkdv_mask map the forward's mask to the one a
    (wrong) backward pass uses; rd_dq replaces the dQ pass's 1/(1-p); l_dropped sums the forward's row sum
    over the dropped P."""

    def __init__(self, dq_mask=None, dkdv_mask=None, rd_dq=None, l_dropped=False, **mask_kw):
        self.dq_mask, self.dkdv_mask, self.rd_dq, self.l_dropped, self.mask_kw = dq_mask, dkdv_mask, rd_dq, l_dropped, mask_kw

    def _run(self, q, k, v, go, bias, scale, causal, p, seed):
        B, Tq, H, _ = q.shape
        M = counter_mask(seed, B, H, Tq, k.shape[1], p, q.device, **self.mask_kw)
        masks = (M, self.dq_mask(M) if self.dq_mask else M, self.dkdv_mask(M) if self.dkdv_mask else M)
        keep = 1 / (1 - p)
        rd = (keep, keep if self.rd_dq is None else self.rd_dq, keep)
        return adr.emulate_passes(q, k, v, go, masks, p, scale, causal, bias, rd=rd, l_dropped=self.l_dropped)

    def forward(self, q, k, v, bias, scale, causal, p, seed):
        return self._run(q, k, v, None, bias, scale, causal, p, seed)[0].to(torch.bfloat16)

    def forward_backward(self, q, k, v, go, bias, scale, causal, p, seed):
        return tuple(t.to(torch.bfloat16) for t in self._run(q, k, v, go, bias, scale, causal, p, seed))


C1, C2, C3, C4 = adr.mfma_cases(64)[:4]
G1 = adr.GENERIC_CASES[0]


@pytest.mark.parametrize("case", [C1, C2, C3, C4, G1], ids=lambda c: c.name)
def test_correct_backend_passes(case):
    m = adr.check_case(EmuBackend(), case, row_ratio=1.5)
    for t in adr.TENSORS:
        assert m[f"F_ratio_{t}"] == 1.0  # the backend is the emulation
        assert m[f"E_fro_{t}"] < 5e-3    # (and the emulation's own error is a fraction of check E's bounds)
    assert m["D_max_rel"] < 2.0 ** -7


def _tail_tile(M):  # the keys of the ragged last 64-key tile take their neighbour's mask bit
    t0 = (M.shape[-1] - 1) // 64 * 64
    out = M.clone()
    out[..., t0:] = M.roll(1, -1)[..., t0:]
    return out


def _one_row(M):  # one query row of one head never dropped
    out = M.clone()
    out[0, 1, 37, :] = True
    return out


FORWARD_CHECKS = {"A", "B", "C", "D"}

WRONG = [  # name, backend, cases, (check, tensor) pairs that must fail, forward checks must pass
    ("dkdv_key_shift", EmuBackend(dkdv_mask=lambda M: M.roll(1, -1)), [C1, C2], [("E", "dK"), ("E", "dV")], True),
    ("dq_ignores_head", EmuBackend(dq_mask=lambda M: M[:, :1].expand_as(M)), [C1, C2], [("E", "dQ")], True),
    ("dq_no_rescale", EmuBackend(rd_dq=1.0), [C1, C2], [("E", "dQ")], True),
    ("dq_tail_tile", EmuBackend(dq_mask=_tail_tile), [C1, C3], [("F", "dQ")], True),
    ("dq_row_unmasked", EmuBackend(dq_mask=_one_row), [C2], [("F", "dQ")], True),
    ("fwd_l_over_dropped", EmuBackend(l_dropped=True), [C1, C4], [("D", "probe values")], False),
    ("mask_period_64", EmuBackend(key_period=64), [C1, C3], [("C", "key+64")], False),
    ("mask_same_heads", EmuBackend(per_head=False), [C1, G1], [("C", "head0_vs_head1")], False),
]


@pytest.mark.parametrize("name,backend,cases,must_fail,forward_ok", WRONG, ids=[w[0] for w in WRONG])
def test_wrong_backend_fails_at_named_check(name, backend, cases, must_fail, forward_ok):
    for case in cases:
        with pytest.raises(adr.CheckFailure) as ei:
            adr.check_case(backend, case, row_ratio=3.0)  # the widest ratio check F may ever get
        failed = ei.value.failed
        for f in must_fail:
            assert f in failed, (case.name, f, failed, str(ei.value))
        if forward_ok:  # a backward-only slip: the probe checks isolate the forward and stay green
            assert not FORWARD_CHECKS & {c for c, _ in failed}, (case.name, failed)
        if must_fail[0][0] == "F":  # the slips only the row-local bound sees: whole-tensor dQ stays in bound
            assert ("E", "dQ") not in failed, (case.name, failed)


def test_probe_recovers_mask_exactly():
    q, k, _, _, _ = adr.make_inputs(C3)
    pd = adr.probe_dropped_probs(EmuBackend(), q, k, None, C3.scale, True, C3.p, C3.seed)
    M = counter_mask(C3.seed, C3.B, C3.H, C3.Tq, C3.Tk, C3.p, "cpu")
    band = ~torch.ones(C3.Tq, C3.Tk, dtype=torch.bool).triu(1 + C3.Tk - C3.Tq)
    assert torch.equal(pd != 0, M & band)


def test_row_err_sees_one_row():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(4, 50, 3, 64, generator=g)
    a = ref + 1e-3 * torch.randn(ref.shape, generator=g)
    base = adr.row_err(a, ref)
    a[1, 7, 2] += 0.3 * ref[1, 7, 2]  # one of 600 rows off by 30 %: 0.3 / sqrt(600) = 1.2e-2 of the whole
    assert adr.rel_fro(a, ref) < 2e-2 and adr.row_err(a, ref) > 100 * base
    ref[0, 0, 0] = 0  # a near-zero reference row does not dominate: the rms floor
    assert adr.row_err(ref + 1e-3, ref) < 2e-3
