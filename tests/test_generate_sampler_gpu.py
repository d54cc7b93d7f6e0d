"""``generate(sampler="native")`` on the GPU: the fused sampler captured together with the decode
step, seeded by the device seed stream of ``ops.rng`` (GPT-2 tiny, bf16)."""

import pytest
import torch

from replicann_amd import ops
from replicann_amd.ops import rng

pytestmark = pytest.mark.gpu

SAMPLED = dict(temperature=0.9, top_k=50, top_p=0.95, sampler="native")


def _model(cuda):
    import replicann_amd as R
    torch.manual_seed(0)
    m = R.GPT2(R.GPT2Config.tiny(n_embd=128, n_head=2, n_layer=2, block_size=128)).to(cuda)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m.eval()


def _prompt(cuda, B=3, T=12):
    return torch.randint(0, 1000, (B, T), generator=torch.Generator().manual_seed(2)).to(cuda)


def test_native_greedy_equals_default_greedy(cuda):
    m, idx = _model(cuda), _prompt(cuda)
    want = m.generate(idx, 20, temperature=0, graph=True)
    assert torch.equal(m.generate(idx, 20, temperature=0, graph=True, sampler="native"), want)
    assert torch.equal(m.generate(idx, 20, temperature=0, graph=False, sampler="native"),
                       m.generate(idx, 20, temperature=0, graph=False))


def test_seeded_runs_and_capture_consumes_no_draws(cuda):
    m, idx = _model(cuda), _prompt(cuda)
    rng.manual_seed(11)
    first = m.generate(idx, 24, graph=True, **SAMPLED)  # captures the step + sampler
    assert len(m._decode_graphs()) == 1
    rng.manual_seed(11)
    second = m.generate(idx, 24, graph=True, **SAMPLED)  # replays the stored graph
    rng.manual_seed(11)
    third = m.generate(idx, 24, graph=True, **SAMPLED)
    assert len(m._decode_graphs()) == 1
    assert first.shape == (3, 36) and torch.equal(first[:, :12], idx) and int(first.max()) < 1000
    assert torch.equal(first, second) and torch.equal(second, third)
    rng.manual_seed(12)
    other = m.generate(idx, 24, graph=True, **SAMPLED)
    assert not torch.equal(first, other)
    # without a reseed the stream moves on
    assert not torch.equal(m.generate(idx, 24, graph=True, **SAMPLED), other)
    # eager: seeded and reproducible as well
    rng.manual_seed(11)
    e1 = m.generate(idx, 8, graph=False, **SAMPLED)
    rng.manual_seed(11)
    assert torch.equal(m.generate(idx, 8, graph=False, **SAMPLED), e1)
    with pytest.raises(ValueError):
        m.generate(idx, 8, generator=torch.Generator(device=cuda), **SAMPLED)


def test_one_sampler_graph_for_every_setting(cuda):
    m, idx = _model(cuda), _prompt(cuda)
    m.generate(idx, 10, temperature=0, graph=True)
    default_keys = list(m._decode_graphs())
    assert len(default_keys) == 1 and len(default_keys[0]) == 5  # as before: no marker
    rng.manual_seed(3)
    outs = [m.generate(idx, 10, graph=True, sampler="native", temperature=t, top_k=k, top_p=p)
            for t, k, p in [(1.0, None, None), (0.7, 5, None), (1.3, None, 0.5), (0.0, None, None), (0.9, 40, 0.9)]]
    keys = list(m._decode_graphs())
    assert len(keys) == 2 and keys[0] == default_keys[0] and keys[1] == default_keys[0] + ("sampler",)
    # the settings reached the stored graph: the greedy call is the default greedy output
    assert torch.equal(outs[3], m.generate(idx, 10, temperature=0, graph=True))
    rng.manual_seed(3)
    again = m.generate(idx, 10, graph=True, sampler="native", temperature=1.0)
    assert torch.equal(again, outs[0])  # ... and back
    m.generate(idx, 10, temperature=0, eos_token_id=5, graph=True, sampler="native")
    assert list(m._decode_graphs())[-1][-2:] == ("ragged", "sampler")
    m.clear_decode_graphs()


@pytest.mark.parametrize("graph", [True, False])
def test_ragged_eos_with_the_native_sampler(cuda, graph):
    m = _model(cuda)
    plens = [12, 5, 9]
    idx = _prompt(cuda)
    greedy, _ = m.generate(idx, 30, temperature=0, prompt_lens=plens, graph=graph)
    eos = int(greedy[1, 5 + 3])  # row 1 emits it as its 4th token (or earlier)
    stop = 5 + greedy[1, 5:].tolist().index(eos) + 1
    want_t, want_l = m.generate(idx, 30, temperature=0, prompt_lens=plens, eos_token_id=eos, pad_token_id=7, graph=graph)
    got_t, got_l = m.generate(idx, 30, temperature=0, prompt_lens=plens, eos_token_id=eos, pad_token_id=7, graph=graph,
                              sampler="native")
    assert int(want_l[1]) == stop and torch.equal(got_t, want_t) and torch.equal(got_l, want_l)
    # sampled: rows stop at their first EOS and are padded from there on; lengths are consistent
    rng.manual_seed(4)
    tok, lens = m.generate(idx, 30, prompt_lens=plens, eos_token_id=eos, pad_token_id=7, graph=graph,
                           temperature=1.5, top_k=8, sampler="native")
    assert tok.shape[1] == int(lens.max())
    for b, p in enumerate(plens):
        n = int(lens[b])
        row = tok[b].tolist()
        assert row[:p] == idx[b, :p].tolist() and p < n <= p + 30
        assert eos not in row[p:n - 1] and (row[n - 1] == eos or n == p + 30)
        assert all(t == 7 for t in row[n:])


def test_frequencies_through_the_seed_path(cuda):
    """4096 rows of one 8-token fp32 row, each drawing hash_uniform(seed, row): every token's count
    within 5 sigma of its probability (the seed is fixed: a deterministic outcome)."""
    row = torch.tensor([0.0, 1.0, -1.0, 2.0, 0.5, -0.5, 1.5, -2.0])
    p = torch.softmax(row.double(), 0)
    x = row.to(cuda).expand(4096, -1).contiguous()
    rng.manual_seed(99)
    tok, kept = ops.sample_logits(x, 1.0, seed_buf=rng.next_seed(cuda))
    assert kept.tolist() == [8] * 4096
    counts = torch.bincount(tok.flatten().cpu(), minlength=8).double()
    sigma = (4096 * p * (1 - p)).sqrt()
    assert bool(((counts - 4096 * p).abs() <= 5 * sigma).all()), (counts, 4096 * p)
