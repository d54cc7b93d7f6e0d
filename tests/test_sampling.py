"""The sampler's reference semantics (``ops.sample_logits`` on CPU tensors: float64 ATen math) —
the oracle the GPU kernel is tested against — and ``generate(sampler="native")`` on a CPU model."""

import pytest
import torch

from replicann_amd import ops
from replicann_amd.models.decoding import _sample
from replicann_amd.ops import sampling

INF = float("inf")


def _row(V, seed):
    x = torch.randn(1, V, generator=torch.Generator().manual_seed(seed)) * 3
    assert x.unique().numel() == V  # tie-free: the two rules agree exactly
    return x


def _torch_kept(x, temperature, top_k, top_p):
    """The set ``decoding._sample``'s filtering leaves finite (its code up to the softmax)."""
    logits = x / temperature
    if top_k is not None and top_k < logits.shape[-1]:
        kth = torch.topk(logits, top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, -INF)
    if top_p is not None and top_p < 1.0:
        srt, idx = torch.sort(logits, dim=-1, descending=True)
        cum = torch.softmax(srt, -1).cumsum(-1)
        drop = cum - torch.softmax(srt, -1) >= top_p
        drop[..., 0] = False
        logits = torch.full_like(logits, -INF).scatter(-1, idx, srt.masked_fill(drop, -INF))
    return torch.isfinite(logits)


@pytest.mark.parametrize("V", [33, 1000])
@pytest.mark.parametrize("top_k, top_p", [(None, None), (5, None), (None, 0.9), (20, 0.8), (2000, 0.5), (1, 0.3)])
def test_kept_set_is_the_default_samplers_on_tie_free_rows(V, top_k, top_p):
    x = _row(V, V)
    for temperature in (1.0, 0.7):
        want = _torch_kept(x.double(), temperature, top_k, top_p)  # float64: no rounding at the top-p boundary
        keep, e = sampling.kept_mask(x, temperature, top_k, top_p)
        assert torch.equal(keep, want)
        assert torch.equal(e > 0, want)
        _, kept = ops.sample_logits(x, temperature, top_k, top_p, u=torch.tensor([0.5]))
        assert int(kept) == int(want.sum())
    # the default sampler only ever returns tokens of that set
    g = torch.Generator().manual_seed(0)
    drawn = torch.cat([_sample(x, 1.0, top_k, g, top_p) for _ in range(32)]).flatten()
    assert bool(_torch_kept(x.double(), 1.0, top_k, top_p)[0, drawn].all())


def test_whole_tie_groups_are_kept():
    # values 4 > 3 = 3 = 3 > 1 = 1 > 0: top_k = 2 cuts inside the group of 3s -> the whole group stays
    x = torch.tensor([[3.0, 1.0, 4.0, 3.0, 0.0, 3.0, 1.0]])
    _, kept = ops.sample_logits(x, 1.0, 2, None, u=torch.tensor([0.0]))
    assert int(kept) == 4
    keep, _ = sampling.kept_mask(x, 1.0, 2, None)
    assert keep.tolist() == [[True, False, True, True, False, True, False]]
    # top-p: p(4) = 0.450, each 3: 0.166.  Mass strictly above the 3s is 0.450 < 0.6 -> all three stay
    # (a cut in sorted order would keep only one of them: 0.450 + 0.166 = 0.616 >= 0.6); above the 1s
    # it is 0.947 >= 0.6 -> both go
    keep, _ = sampling.kept_mask(x, 1.0, None, 0.6)
    assert keep.tolist() == [[True, False, True, True, False, True, False]]
    # top_p below the top token's own mass: it stays alone
    keep, _ = sampling.kept_mask(x, 1.0, None, 0.01)
    assert keep.tolist() == [[False, False, True, False, False, False, False]]
    # top-p applies inside the top-k set: with k = 1 the 4 has all the mass
    assert int(ops.sample_logits(x, 1.0, 1, 0.99, u=torch.tensor([0.3]))[1]) == 1


def test_draw_edges():
    x = torch.tensor([[-INF, 0.5, -INF, 2.0, 1.0, -INF]])
    first, _ = ops.sample_logits(x, 1.0, None, None, u=torch.tensor([0.0]))
    last, kept = ops.sample_logits(x, 1.0, None, None, u=torch.tensor([1 - 2.0 ** -24]))
    assert int(first) == 1 and int(last) == 4  # never a -inf logit, at either end
    assert int(kept) == 6  # no filter: every token passes, -inf ones with zero mass
    for u in torch.linspace(0, 1 - 2.0 ** -24, 50):
        tok, _ = ops.sample_logits(x, 0.5, None, None, u=u.reshape(1))
        assert int(tok) in (1, 3, 4)
    # index-order inverse CDF: masses e^0, e^1 at indices 0, 1 -> the boundary is at 1 / (1 + e)
    y = torch.tensor([[0.0, 1.0]])
    edge = 1 / (1 + torch.e)
    assert int(ops.sample_logits(y, 1.0, None, None, u=torch.tensor([edge - 1e-4]))[0]) == 0
    assert int(ops.sample_logits(y, 1.0, None, None, u=torch.tensor([edge + 1e-4]))[0]) == 1
    # one finite logit
    z = torch.full((1, 9), -INF)
    z[0, 6] = -3.0
    for u in (0.0, 0.7, 1 - 2.0 ** -24):
        assert int(ops.sample_logits(z, 1.0, 3, 0.5, u=torch.tensor([u]))[0]) == 6


def test_greedy_and_all_equal():
    x = torch.tensor([[1.0, 7.0, 7.0, -2.0, 7.0], [5.0, 5.0, 5.0, 5.0, 5.0]])
    tok, kept = ops.sample_logits(x, 0.0, 3, 0.5, u=torch.tensor([0.9, 0.9]))
    assert tok.tolist() == [[1], [0]] and kept.tolist() == [1, 1]  # lowest index on ties
    assert tok.dtype == torch.int64 and kept.dtype == torch.int32 and tok.shape == (2, 1)
    eq = torch.full((1, 77), 0.25)
    for top_k, top_p in [(None, None), (5, None), (None, 0.3), (5, 0.3)]:  # one tie group: all or nothing
        tok, kept = ops.sample_logits(eq, 0.8, top_k, top_p, u=torch.tensor([0.5]))
        assert int(kept) == 77 and int(tok) == 38
    assert int(ops.sample_logits(eq, 0.8, None, None, u=torch.tensor([0.0]))[0]) == 0
    assert int(ops.sample_logits(eq, 0.8, None, None, u=torch.tensor([1 - 2.0 ** -24]))[0]) == 76


def test_params_tensor_and_argument_checks():
    x = _row(33, 5)
    u = torch.tensor([0.3])
    a = ops.sample_logits(x, 0.7, 5, 0.9, u=u)
    b = ops.sample_logits(x, u=u, params=torch.tensor([0.7, 5.0, 0.9]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        ops.sample_logits(x, 1.0)  # neither u nor seed_buf
    with pytest.raises(ValueError):
        ops.sample_logits(x, 1.0, u=u, seed_buf=torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError):
        ops.sample_logits(x, 1.0, None, 0.0, u=u)
    with pytest.raises(ValueError):
        ops.sample_logits(x, -1.0, u=u)


def test_hash_uniform_matches_its_definition():
    # splitmix64 finaliser of seed + γ·(idx + 1), top 24 bits: a multiple of 2^-24 in [0, 1)
    for seed, idx in [(0, 0), (12345, 7), ((1 << 62) - 1, 63)]:
        v = sampling.hash_uniform(seed, idx)
        assert 0.0 <= v < 1.0 and v * 2 ** 24 == int(v * 2 ** 24)
    assert sampling.hash_uniform(1, 0) != sampling.hash_uniform(1, 1) != sampling.hash_uniform(2, 1)


def _tiny():
    import replicann_amd as R
    torch.manual_seed(0)
    return R.GPT2(R.GPT2Config.tiny(n_embd=64, n_head=2, n_layer=2, block_size=64)).eval()


def test_generate_native_on_cpu():
    m = _tiny()
    idx = torch.randint(0, m.config.vocab_size, (2, 5), generator=torch.Generator().manual_seed(1))
    kw = dict(temperature=0.9, top_k=20, top_p=0.9, sampler="native")
    a = m.generate(idx, 6, generator=torch.Generator().manual_seed(3), **kw)
    b = m.generate(idx, 6, generator=torch.Generator().manual_seed(3), **kw)
    c = m.generate(idx, 6, generator=torch.Generator().manual_seed(4), **kw)
    assert a.shape == (2, 11) and torch.equal(a[:, :5], idx)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(m.generate(idx, 6, temperature=0), m.generate(idx, 6, temperature=0, sampler="native"))
    # ragged + EOS keeps its bookkeeping with the native sampler
    greedy = m.generate(idx, 6, temperature=0)
    eos = int(greedy[0, 7])
    t0, l0 = m.generate(idx, 6, temperature=0, eos_token_id=eos)
    t1, l1 = m.generate(idx, 6, temperature=0, eos_token_id=eos, sampler="native")
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    with pytest.raises(ValueError):
        m.generate(idx, 3, sampler="fast")
