"""The LayerNorm backward kernel writing the e5m2 dY of the fp8 projection that produced its input
(csrc/kernels/layernorm.hip ln_bwd_k<.., Q8>, ops/norm.py producer_fp8): the bytes and the delayed-scaling slot
must be exactly what the projection's own quantisation pass (bf8_quantize, delayed) makes from the stored bf16
dx, so a training step is bitwise the same with and without it."""

import pytest
import torch

import replicann_amd.ops.norm as norm_mod
from replicann_amd.models.gpt2 import GPT2, GPT2Config

pytestmark = pytest.mark.gpu


def test_layernorm_bwd_q8_matches_quantisation_pass(cuda):
    torch.manual_seed(3)
    M, E = 4096, 1024
    dy = torch.randn(M, E, device=cuda).bfloat16()
    gh = torch.randn(M, E, device=cuda).bfloat16()
    h = torch.randn(M, E, device=cuda).bfloat16()
    w = (torch.rand(E, device=cuda) + 0.5).bfloat16()
    mean = h.float().mean(1)
    rstd = torch.rsqrt(h.float().var(1, unbiased=False) + 1e-5)
    ops = torch.ops.replicann
    slot = torch.tensor([0.0, 3.0, 0.0, 0.0], device=cuda)  # a seeded slot: amax 3 from "the previous step"
    slot_ref = slot.clone()
    q8 = torch.empty(M, E, dtype=torch.uint8, device=cuda)
    dx, _, _ = ops.layernorm_bwd(dy, gh, h, w, mean, rstd, None, None, None, q8, slot)
    dx_ref, _, _ = ops.layernorm_bwd(dy, gh, h, w, mean, rstd, None, None, None)
    q_ref = ops.bf8_quantize(dx_ref, slot_ref, True)
    assert torch.equal(dx, dx_ref)
    assert torch.equal(q8, q_ref.view(M, E))
    assert torch.equal(slot, slot_ref)  # same rolled scale, same recorded amax


def _step_grads(cuda, ln_q8, steps=3):
    from replicann_amd.utils.flat import FlatParams

    torch.manual_seed(0)
    m = GPT2(GPT2Config.tiny(fp8=True, n_embd=256, vocab_size=2000, vocab_pad=2048)).to(cuda)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    # the training path: gradients accumulated in place into the flat buffer (the token-embedding scatter
    # then honours REPLICANN_DETERMINISTIC; the standalone embedding_bwd adds float atomics in arrival order)
    flat = FlatParams(m)
    idx = torch.randint(0, 2000, (4, 128), device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    old = norm_mod.FP8_LN_Q8
    norm_mod.FP8_LN_Q8 = ln_q8
    try:
        for _ in range(steps):  # step 1 seeds the gradient slots; later steps take the fused path
            flat.zero_grad()
            m(idx, idx).backward()
    finally:
        norm_mod.FP8_LN_Q8 = old
    return m, [flat.grad.clone()]


def _linear_ln_backward(cuda, wgrad, token_counts):
    """An fp8 Linear(128, 128) feeding a LayerNorm wired as PreLNBlock wires a projection to the next LayerNorm
    (``producer_bias`` / ``producer_fp8``), fp8 weight gradient per ``wgrad``, data gradient in bf16.  One warm-up
    forward/backward at 256 tokens seeds the delayed gradient scale; then one forward per entry of
    ``token_counts`` and ONE backward on the summed losses.  Returns (state, gradient slot after the warm-up,
    gradient slot after the backward, weight gradient, the inputs' gradients)."""
    from replicann_amd.models import blocks
    from replicann_amd.utils.flat import FlatParams

    torch.manual_seed(0)
    net = torch.nn.Module()
    net.lin, net.ln = blocks.Linear(128, 128, fp8=True), blocks.LayerNorm(128)
    net.to(cuda)
    for p in net.parameters():
        p.data = p.data.to(torch.bfloat16)
    st = net.lin.fp8_state
    st.wgrad, st.dgrad = wgrad, False
    flat = FlatParams(net)

    def call(n, seed):  # the same n and seed: the same data, whatever ran before
        gen = torch.Generator(device=cuda).manual_seed(seed)
        x = torch.randn(n, 128, device=cuda, generator=gen).bfloat16().requires_grad_()
        g = torch.randn(n, 128, device=cuda, generator=gen)
        y, _ = net.ln(net.lin(x), return_sum=True, producer_bias=net.lin.bias, producer_fp8=st)
        return x, (y.float() * g).sum()

    flat.zero_grad()
    call(256, 1000)[1].backward()
    warm = net.lin.fp8_gscales.clone()
    flat.zero_grad()
    xs, losses = zip(*[call(n, n) for n in token_counts])
    sum(losses).backward()
    return st, warm, net.lin.fp8_gscales.clone(), net.lin.weight.grad.clone(), [x.grad.clone() for x in xs]


def test_two_forwards_before_one_backward_each_act_on_their_own_plan(cuda):
    """an fp8 layer run twice before one backward (300 tokens: no fp8 weight gradient; then 256
    tokens: fp8 weight gradient).  Each call's LayerNorm backward must act on the plan of ITS call's forward:
    the 300-token call's must neither roll the layer's gradient scale slot nor leave an e5m2 dY on offer that
    its linear (bf16 gradients) never takes.  Read from the layer's live state at backward time instead, both
    calls see the 256-token plan: the slot rolls twice and an offer is left pending."""
    st, warm, slot, gw, gxs = _linear_ln_backward(cuda, True, (300, 256))
    assert st._offer is None and st._goffer is None
    # the slot advanced once per call that took an fp8 gradient: exactly as after the 256-token call alone
    st1, warm1, slot1, _, _ = _linear_ln_backward(cuda, True, (256,))
    assert st1._offer is None and st1._goffer is None
    assert torch.equal(warm, warm1)
    assert not torch.equal(slot1, warm1)
    assert torch.equal(slot, slot1), (warm, slot, slot1)
    # and the gradients are the bf16-weight-gradient ones within the fp8 weight-gradient bound of the model test
    # (tests/test_fp8_wgrad_gpu.py test_fp8_model_wgrad_tracks_bf16_wgrad: relative Frobenius error < 0.08)
    _, _, _, gw0, gxs0 = _linear_ln_backward(cuda, False, (300, 256))
    for a, b in zip([gw, *gxs], [gw0, *gxs0]):
        assert torch.isfinite(a.float()).all()
        assert ((a.float() - b.float()).norm() / b.float().norm()).item() < 0.08


def test_gpt2_fp8_step_bitwise_with_layernorm_e5m2(cuda, monkeypatch):
    # the default token-embedding scatter adds float atomics in arrival order (a repeated token id's rows sum
    # in whatever order the waves land): two runs whose earlier kernels differ in timing may differ in wte's
    # last bits.  The fixed-point scatter is order-independent, so the comparison is bitwise everywhere.
    monkeypatch.setenv("REPLICANN_DETERMINISTIC", "1")
    m1, g1 = _step_grads(cuda, True)
    m0, g0 = _step_grads(cuda, False)
    assert m1.h[0].attn.c_proj.fp8_state is not None and m1.h[0].attn.c_proj.fp8_state.g_ready
    for a, b in zip(g1, g0):
        assert torch.equal(a, b)
    for b1, b0 in zip(m1.buffers(), m0.buffers()):
        assert torch.equal(b1, b0)
