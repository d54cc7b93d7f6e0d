"""Attention dropout on the HIP kernels — forward, dQ and dK/dV, every <CAUSAL, BIAS, DROP=true> form of
every MFMA head size, the generic scalar kernels, the packed-QKV path and the host-seed entry points —
against a float64 reference that uses the mask read out of the forward kernel itself
(tests/attn_dropout_ref.py: the one-hot-V probe and checks A to F), and the elementwise dropout's backward
against its forward's mask."""

import pytest
import torch

import attn_dropout_ref as adr
from replicann_amd import ops
from replicann_amd.ops import rng

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _rng_restored():
    """The seeds set here do not leak into the tests that run afterwards."""
    base, states = rng._BASE[0], rng.state_dict()
    yield
    rng._BASE[0] = base
    rng.load_state_dict(states)


class OpsBackend:
    """The public path: ops.rng.manual_seed(seed) before each ops.attention call, so the probe calls and the
    real call draw the same device seed (the kernels read it through seed_ptr)."""

    def forward(self, q, k, v, bias, scale, causal, p, seed):
        rng.manual_seed(seed)
        with torch.no_grad():
            return ops.attention(q, k, v, scale=scale, causal=causal, bias=bias, dropout_p=p, training=True)

    def forward_backward(self, q, k, v, go, bias, scale, causal, p, seed):
        qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
        rng.manual_seed(seed)
        o = ops.attention(qg, kg, vg, scale=scale, causal=causal, bias=bias, dropout_p=p, training=True)
        o.backward(go)
        return o.detach(), qg.grad, kg.grad, vg.grad


class HostSeedBackend:
    """The raw entry points with an integer seed and no seed buffer."""

    def forward(self, q, k, v, bias, scale, causal, p, seed):
        return torch.ops.replicann.attn_fwd(q, k, v, bias, scale, causal, p, seed, None)[0]

    def forward_backward(self, q, k, v, go, bias, scale, causal, p, seed):
        o, lse = torch.ops.replicann.attn_fwd(q, k, v, bias, scale, causal, p, seed, None)
        dq, dk, dv = torch.ops.replicann.attn_bwd(go, q, k, v, o, lse, bias, scale, causal, p, seed, None)
        return o, dq, dk, dv


class PackedBackend:
    """ops.attention_packed on a (B, T, 3, H, D) tensor whose projection bias is a FlatParams parameter: the
    strided-output backward launch with the in-kernel column partials of dQKV.  Keeps the last backward's
    packed dQKV and bias gradient."""

    def _pack(self, q, k, v):
        return torch.stack((q, k, v), dim=2).contiguous()

    def forward(self, q, k, v, bias, scale, causal, p, seed):
        rng.manual_seed(seed)
        with torch.no_grad():  # the probe replaces qkv[:, :, 2]
            return ops.attention_packed(self._pack(q, k, v), scale=scale, causal=causal, bias=bias, dropout_p=p,
                                        training=True)

    def forward_backward(self, q, k, v, go, bias, scale, causal, p, seed):
        from replicann_amd.utils.flat import FlatParams
        B, T, H, D = q.shape
        mod = torch.nn.Module()
        mod.pb = torch.nn.Parameter(torch.zeros(3 * H * D, device=q.device).bfloat16())
        flat = FlatParams(mod)
        flat.zero_grad()
        qkv = self._pack(q, k, v).requires_grad_()
        rng.manual_seed(seed)
        o = ops.attention_packed(qkv, scale=scale, causal=causal, bias=bias, dropout_p=p, training=True,
                                 producer_bias=mod.pb)
        o.backward(go)
        assert mod.pb._rn_bias_done
        self.dqkv, self.pb_grad, self._keep = qkv.grad, mod.pb.grad, (mod, flat)
        dq, dk, dv = qkv.grad.unbind(2)
        return o.detach(), dq, dk, dv


@pytest.mark.parametrize("D", [32, 64, 128])
@pytest.mark.parametrize("i", range(6), ids=[c.name[:2] for c in adr.mfma_cases(0)])
def test_attention_dropout_mfma(cuda, D, i):
    """Cases 1 to 6 (attn_dropout_ref.mfma_cases): causal / non-causal, causal offset with 5 key tiles, bias
    with Tq > Tk, the reference decoder's tril bias, batched bias with -inf entries; several key tiles, a ragged
    tail, more than one forward workgroup per head.  (Case 2 at D = 64 has Tq, Tk <= 256: taking the
    whole-head-resident path, which has no dropout, fails check B.)"""
    assert ops.attention_is_mfma(D)
    adr.check_case(OpsBackend(), adr.mfma_cases(D)[i], device=cuda)


@pytest.mark.parametrize("case", adr.GENERIC_CASES, ids=lambda c: c.name)
def test_attention_dropout_generic(cuda, case):
    """The scalar kernels' dropout branches (forward, dQ per query row, dK/dV per key row)."""
    assert not ops.attention_is_mfma(case.D)
    adr.check_case(OpsBackend(), case, device=cuda)


def test_attention_dropout_packed(cuda):
    """Checks A to F on the packed dQKV, and the projection's bias gradient — the kernels' column partials under
    dropout — against Σ_rows of that dQKV."""
    be, c = PackedBackend(), adr.PACKED_CASE
    adr.check_case(be, c, device=cuda)
    ref = be.dqkv.float().reshape(c.B * c.Tq, 3 * c.H * c.D).sum(0)
    err = adr.rel_fro(be.pb_grad, ref)
    assert err < 1e-2, err


def test_attention_dropout_host_seed(cuda):
    """MFMA case 1 at D = 64 through attn_fwd / attn_bwd with an integer seed (seed_buf = None)."""
    adr.check_case(HostSeedBackend(), adr.mfma_cases(64)[0], device=cuda)


@pytest.mark.parametrize("shape", [(1000, 300), (100003,)], ids=["1000x300", "flat100003"])
def test_dropout_backward_uses_forward_mask(cuda, shape):
    """ops.dropout's backward re-runs the forward kernel on the gradient with the saved seed: the zero pattern
    of x.grad is the zero pattern of y (x and g are clamped away from zero, so both patterns are the mask), kept
    entries are x/(1-p) and g/(1-p) to one bf16 rounding, and the mask has the keep rate and no structure
    (checks B and C: neighbouring elements, neighbouring rows) — vector body and scalar tail."""
    p = 0.25
    gen = torch.Generator().manual_seed(31)

    def away_from_zero():
        t = torch.randn(shape, generator=gen)
        return (torch.sign(t) * t.abs().clamp_min(0.5)).to(torch.bfloat16).to(cuda)

    x, g = away_from_zero().requires_grad_(), away_from_zero()
    rng.manual_seed(adr.SEED)
    y = ops.dropout(x, p, True)
    y.backward(g)
    M = y.detach() != 0
    assert torch.equal(x.grad != 0, M)
    for got, src in ((y.detach(), x.detach()), (x.grad, g)):
        want = src.double() / (1 - p)
        rel = ((got.double() - want).abs() / want.abs())[M].max().item()
        assert rel <= 2.0 ** -8, rel
    vis = torch.ones_like(M)
    rate, n, dev = adr.keep_rate(M, vis, p)
    assert dev <= adr.SIGMAS, (rate, n, dev)
    flatM = M.reshape(-1)
    structure = adr.mask_structure(flatM, torch.ones_like(flatM), p, [("element+1", 0, 1)])
    if M.dim() == 2:
        structure.update(adr.mask_structure(M, vis, p, [("row+1", 0, 1)]))
    assert len(structure) == M.dim()
    for name, (ag, pairs, d) in structure.items():
        assert d <= adr.SIGMAS, (name, ag, pairs, d)
