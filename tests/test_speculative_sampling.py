"""Speculative sampling on the CPU: the float64 reference of ``ops.speculative_verify`` on hand-checked
cases, the exactness of the accept / resample rule on a deterministic grid of uniforms (no random
tolerance), and ``generate(draft=..., sampler="native")`` on the fp32 models of test_speculative.py.

The grid test: with N midpoints per uniform every probability the grid realises is off by at most half a
cell per CDF edge, which bounds the marginal's error by 2 / N per component (a numpy model of the rule
stayed at 1.12 / N over 200 random pairs, zeros in p or q included)."""

import math

import pytest
import torch

import replicann_amd as R
from replicann_amd import ops
from replicann_amd.models.decoding import accept, sampler_params
from replicann_amd.ops import sampling, speculative

PLENS = [5, 20, 13]
NEW = 12
NINF = float("-inf")


def _logp(*rows):
    """Rows of probabilities as logits (log p; 0 → -inf): at temperature 1 the distribution is the row."""
    return torch.tensor([[math.log(v) if v > 0 else NINF for v in r] for r in rows], dtype=torch.float32)


def _verify(p_rows, q_rows, drafts, u, temperature=1.0, top_k=None, top_p=None, **kw):
    """One batch row: target rows p (K+1 of them), draft rows q (K), u as [(u_acc, u_draw)] per position."""
    t = (p_rows if torch.is_tensor(p_rows) else _logp(*p_rows)).unsqueeze(0)
    d = (q_rows if torch.is_tensor(q_rows) else _logp(*q_rows)).unsqueeze(0)
    tok, m = ops.speculative_verify(t, d, torch.tensor([drafts]), temperature, top_k, top_p,
                                    u=torch.tensor([u], dtype=torch.float32), **kw)
    assert tok.dtype == torch.long and m.dtype == torch.long and tok.shape == (1, len(drafts) + 1)
    return tok[0].tolist(), int(m[0])


P, Q = [0.5, 0.3, 0.2], [0.2, 0.5, 0.3]
U_GRID = [0.0, 0.1, 0.5, 0.59, 0.61, 0.9, 0.99999994]


# ------------------------------------------------------------------ the reference, by hand
def test_hand_checked_acceptance_threshold_and_residual():
    # d = 1: accepted iff u · 0.5 < 0.3; the residual max(p - q, 0) = [0.3, 0, 0] is token 0 whatever u_draw
    for u in U_GRID:
        for ud in (0.0, 0.5, 0.99):
            tok, a = _verify([P, P], [Q], [1], [(u, ud), (0.3, 0.6)])
            if u < 0.6:  # accepted: the bonus token from p_1 at 0.6: cdf 0.5, 0.8 → token 1
                assert (tok, a) == ([1, 1], 1), u
            else:
                assert (tok, a) == ([0, 0], 0), u
    # d = 0: p(d) > q(d): accepted for every u
    for u in U_GRID:
        assert _verify([P, P], [Q], [0], [(u, 0.0), (0.3, 0.95)]) == ([0, 2], 1)


def test_equal_distributions_accept_for_every_u():
    g = torch.Generator().manual_seed(0)
    t = torch.randn(4, 8, generator=g)
    for u in U_GRID:
        for d in range(8):
            tok, a = _verify(t, t[:3].clone(), [d, (d + 3) % 8, 7 - d], [(u, 0.5)] * 4, temperature=0.7)
            assert a == 3 and tok[:3] == [d, (d + 3) % 8, 7 - d], (u, d)


def test_draft_outside_the_targets_top_k_is_rejected_and_replaced_from_the_kept_set():
    t = torch.tensor([[3.0, 2.0, 1.0, 0.0, -1.0, -2.0]] * 2)
    d = torch.tensor([[0.0, 0.0, 5.0, 4.0, 0.0, 0.0]])
    for u in U_GRID:
        for ud in U_GRID:
            tok, a = _verify(t, d, [2], [(u, ud), (0.5, 0.5)], top_k=2)  # q(2) > 0 = p(2)
            assert a == 0 and tok[0] in (0, 1) and tok[1] == 0, (u, ud)


def test_all_accepted_row_ends_with_a_bonus_token_from_the_last_target_row():
    g = torch.Generator().manual_seed(1)
    t = torch.randn(3, 8, generator=g)
    d = [int(t[0].topk(2).indices[1]), int(t[1].argmax())]  # tokens inside the top-5 of their rows
    for ud in U_GRID:
        tok, a = _verify(t, t[:2].clone(), d, [(0.5, 0.1), (0.5, 0.2), (0.9, ud)], temperature=1.3, top_k=5)
        want = sampling.reference(t[2:3], 1.3, 5, 1.0, torch.tensor([ud]))[0]
        assert a == 2 and tok == d + [int(want)], ud


def test_a_token_the_drafts_filter_would_not_emit_is_rejected():
    # q(d) = 0 (d outside the draft's top-2) although p(d) is large and u = 0
    tok, a = _verify([[0.1, 0.1, 0.8], P], [[0.5, 0.4, 0.1]], [2], [(0.0, 0.0), (0.5, 0.5)], top_k=2)
    assert a == 0 and tok == [2, 0]  # the residual max(p - q, 0) with q = [5/9, 4/9, 0] is [0, 0, 0.8]
    # a -inf draft logit: the same
    tok, a = _verify([P, P], [[0.5, 0.5, 0.0]], [2], [(0.0, 0.5), (0.5, 0.5)])
    assert a == 0 and tok == [2, 0]  # the residual is [0, 0, 0.2] (up to the rounding of log 0.3 + log 0.2 at index 0)


def test_zero_residual_falls_back_to_the_target_distribution():
    # p = q on the kept set {0, 1}; d = 2 is outside it: rejected, the residual is all zero: a draw from p
    row = [0.5, 0.3, 0.2]
    for ud in U_GRID:
        tok, a = _verify([row, row], [row], [2], [(0.0, ud), (0.5, 0.5)], top_k=2)
        want = sampling.reference(_logp(row), 1.0, 2, 1.0, torch.tensor([ud]))[0]
        assert a == 0 and tok == [int(want), 0], ud


def test_temperature_zero_equals_accept_on_the_argmaxes():
    g = torch.Generator().manual_seed(2)
    t = torch.randn(6, 5, 8, generator=g)
    d = torch.randn(6, 4, 8, generator=g)
    top = t.argmax(-1)
    drafts = top[:, :4].clone()
    drafts[0, 0] = (drafts[0, 0] + 1) % 8  # a = 0
    drafts[1, 2] = (drafts[1, 2] + 1) % 8  # a = 2, a later match does not count
    drafts[2, 3] = (drafts[2, 3] + 1) % 8
    drafts[3] = torch.randint(0, 8, (4,), generator=g)
    tok, m = ops.speculative_verify(t, d, drafts, 0.0, u=torch.rand(6, 5, 2, generator=g))
    count, want, a = accept(drafts, top, pad=0)
    assert torch.equal(m, a) and torch.equal(tok, want) and m.tolist()[:3] == [0, 2, 3] and int(m[4]) == 4
    t[5, 0, 3] = t[5, 0].max()  # ties: the lowest index; NaN counts as -inf
    t[5, 0, 6] = t[5, 0].max()
    t[5, 1, 0] = float("nan")
    tok2, _ = ops.speculative_verify(t, d, drafts, 0.0, u=torch.rand(6, 5, 2, generator=g))
    x = torch.where(t.isnan(), torch.full_like(t, NINF), t)
    assert torch.equal(tok2, accept(drafts, x.argmax(-1), pad=0)[1])


def test_params_override_the_settings():
    g = torch.Generator().manual_seed(3)
    t, d = torch.randn(5, 3, 8, generator=g), torch.randn(5, 2, 8, generator=g)
    drafts = torch.randint(0, 8, (5, 2), generator=g)
    u = torch.rand(5, 3, 2, generator=g)
    for setting in ((0.7, 3, 0.9), (1.3, None, None), (0.0, None, None)):
        want = ops.speculative_verify(t, d, drafts, *setting, u=u)
        got = ops.speculative_verify(t, d, drafts, 1.0, u=u, params=sampler_params(*setting))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(ops.speculative_verify(t, d, drafts, 1.0, u=u)[0],
                           ops.speculative_verify(t, d, drafts, 1.0, u=u, params=sampler_params(0.0, None, None))[0])


def test_argument_errors():
    t, d = torch.zeros(2, 3, 8), torch.zeros(2, 2, 8)
    drafts, u = torch.zeros(2, 2, dtype=torch.long), torch.zeros(2, 3, 2)
    assert ops.speculative_verify(t, d, drafts, 1.0, u=u)[0].shape == (2, 3)
    bad = [
        dict(t=torch.zeros(2, 1, 8), d=torch.zeros(2, 0, 8), drafts=torch.zeros(2, 0, dtype=torch.long)),  # K = 0
        dict(t=torch.zeros(2, 17, 8), d=torch.zeros(2, 16, 8), drafts=torch.zeros(2, 16, dtype=torch.long)),  # K = 16
        dict(d=torch.zeros(2, 3, 8)), dict(d=torch.zeros(2, 2, 7)), dict(drafts=torch.zeros(2, 3, dtype=torch.long)),
        dict(t=t[0]), dict(d=d.double()), dict(drafts=drafts.int()),
        dict(u=None), dict(u=u, seed_buf=torch.zeros(1, dtype=torch.long)), dict(u=None, seed_buf=torch.zeros(1, dtype=torch.long)),
        dict(u=torch.zeros(2, 3)), dict(drafts=drafts + 8), dict(drafts=drafts - 1),
        dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
    ]
    for kw in bad:
        a = dict(t=t, d=d, drafts=drafts, temperature=1.0, top_k=None, top_p=None, u=u, seed_buf=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.speculative_verify(a["t"], a["d"], a["drafts"], a["temperature"], a["top_k"], a["top_p"], u=a["u"],
                                   seed_buf=a["seed_buf"])


# ------------------------------------------------------------------ exactness of the rule, on a grid
N = 64
GRID = (torch.arange(N, dtype=torch.float64) + 0.5) / N


def _pairs():
    g = torch.Generator().manual_seed(4)
    out = [(torch.randn(7, generator=g) * 1.5, torch.randn(7, generator=g) * 1.5, None) for _ in range(4)]
    p, q = torch.randn(7, generator=g), torch.randn(7, generator=g)
    p[[1, 4]] = NINF  # zeros in p: those drafts are always rejected
    out.append((p, q, None))
    p, q = torch.randn(7, generator=g), torch.randn(7, generator=g)
    q[[0, 2, 5]] = NINF  # zeros in q: the residual keeps all of p there
    out.append((p, q, None))
    p, q = torch.randn(7, generator=g), torch.randn(7, generator=g)
    p[3] = NINF
    q[[3, 6]] = NINF
    out.append((p, q, None))
    out.append((torch.randn(7, generator=g) * 2, torch.randn(7, generator=g) * 2, 3))  # top-k on both sides
    out.append((torch.tensor([0.0, 1, 2, 3, 4, 5, 6]), torch.tensor([6.0, 5, 4, 3, 2, 1, 0]), 3))  # disjoint top-3 sets
    return out


@pytest.mark.parametrize("case", range(9))
def test_first_committed_token_is_distributed_as_the_target(case):
    """V = 7, K = 1, N = 64 midpoints for each of the draft draw, the acceptance and the resample: the
    marginal of the first committed token over the 64³ grid is p within 2 / N in every component."""
    lp, lq, top_k = _pairs()[case]
    T = 0.9
    p = speculative._probs(lp.view(1, 7), T, top_k, None)[0]
    d = sampling.reference(lq.view(1, 7).expand(N, 7), T, top_k, None, GRID)[0][:, 0]  # the draft's draws from q
    ua, ud = torch.meshgrid(GRID, GRID, indexing="ij")
    u = torch.stack([torch.stack([ua.reshape(-1), ud.reshape(-1)], 1), torch.full((N * N, 2), 0.5, dtype=torch.float64)], 1)
    marginal = torch.zeros(7, dtype=torch.float64)
    for tok in d.unique().tolist():
        weight = float((d == tok).sum()) / N
        first = ops.speculative_verify(lp.view(1, 1, 7).expand(N * N, 2, 7), lq.view(1, 1, 7).expand(N * N, 1, 7),
                                       torch.full((N * N, 1), tok), T, top_k, None, u=u)[0][:, 0]
        marginal += weight * torch.bincount(first, minlength=7).double() / (N * N)
    assert abs(float(marginal.sum()) - 1.0) < 1e-12
    err = (marginal - p).abs().max().item()
    assert err <= 2.0 / N, (err * N, marginal.tolist(), p.tolist())
    assert bool((marginal[p == 0] == 0).all())  # a token outside the target's kept set is never committed


# ------------------------------------------------------------------ generate(draft=..., sampler="native")
def _model(seed=0, **kw):
    torch.manual_seed(seed)
    cfg = dict(n_embd=128, n_head=4, n_layer=2, block_size=128)
    cfg.update(kw)
    return R.GPT2(R.GPT2Config.tiny(**cfg)).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def other():
    return _model(seed=7)


def _padded(seed=1, junk=False):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 1000, (len(PLENS), max(PLENS)), generator=g)
    pad = torch.arange(max(PLENS)).unsqueeze(0) >= torch.tensor(PLENS).unsqueeze(1)
    fill = torch.randint(0, 1000, idx.shape, generator=g) if junk else torch.zeros_like(idx)
    return torch.where(pad, fill, idx)


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("which", ["same", "other"])
def test_top_k_1_sampling_equals_plain_greedy(model, other, k, which):
    """top_k = 1 leaves one token (no ties at the maximum in fp32): p and q are one-hot, whatever the uniforms."""
    draft = model if which == "same" else other
    kw = dict(temperature=0.8, top_k=1, sampler="native", draft=draft, draft_k=k)
    idx = _padded()[:, :5]
    stats = {}
    out = model.generate(idx, NEW, generator=_gen(), stats=stats, **kw)
    assert torch.is_tensor(out) and torch.equal(out, model.generate(idx, NEW, temperature=0))
    assert (NEW - 1 + k) // (k + 1) <= stats["rounds"] <= NEW - 1
    assert all(0 <= a <= d for a, d in zip(stats["accepted"].tolist(), stats["drafted"].tolist()))
    if which == "same":
        assert stats["accepted"].tolist() == stats["drafted"].tolist() == [k * stats["rounds"]] * 3
    base, blens = model.generate(_padded(), NEW, temperature=0, prompt_lens=PLENS)
    tokens, lens = model.generate(_padded(junk=True), NEW, prompt_lens=PLENS, generator=_gen(1), **kw)
    assert torch.equal(tokens, base) and torch.equal(lens, blens)
    eos = int(base[1, PLENS[1] + 3])
    want, wlens = model.generate(_padded(), NEW, temperature=0, prompt_lens=PLENS, eos_token_id=eos, pad_token_id=0)
    got, glens = model.generate(_padded(), NEW, prompt_lens=PLENS, eos_token_id=eos, pad_token_id=0, generator=_gen(2), **kw)
    assert torch.equal(glens, wlens) and torch.equal(got, want)


@pytest.mark.parametrize("which", ["same", "other"])
def test_sampled_tokens_are_among_the_targets_top_5(model, other, which):
    draft = model if which == "same" else other
    kw = dict(temperature=0.8, top_k=5, sampler="native", draft=draft, draft_k=4, prompt_lens=PLENS)
    stats = {}
    tokens, lens = model.generate(_padded(), NEW, generator=_gen(5), stats=stats, **kw)
    assert lens.tolist() == [p + NEW for p in PLENS] and tokens.shape == (3, max(PLENS) + NEW)
    for b, p in enumerate(PLENS):
        assert torch.equal(tokens[b, :p], _padded()[b, :p]) and bool((tokens[b, p + NEW:] == 0).all())
        with torch.no_grad():
            full = model(tokens[b: b + 1, : int(lens[b])])[0]
        for t in range(p, int(lens[b])):
            lg = full[t - 1]
            assert lg[tokens[b, t]] >= lg.topk(5).values[-1] - 3e-2 * lg.abs().max(), (b, t)
    # equal generators: equal outputs; another seed: sampling is really on (some token differs)
    again, _ = model.generate(_padded(), NEW, generator=_gen(5), **kw)
    assert torch.equal(again, tokens)
    differs, _ = model.generate(_padded(), NEW, generator=_gen(6), **kw)
    assert not torch.equal(differs, tokens)
    assert 1 <= stats["rounds"] <= NEW - 1
    drafted, accepted = stats["drafted"].tolist(), stats["accepted"].tolist()
    # a row drafts 4 tokens in every round in which it is live, and some row is live in every round
    assert all(d % 4 == 0 for d in drafted) and max(drafted) == 4 * stats["rounds"]
    assert all(0 <= a <= d for a, d in zip(accepted, drafted))
    # the committed tokens of a row: the first from the prefill, then at most matched + 1 per live round
    assert all(a + d // 4 >= NEW - 1 for a, d in zip(accepted, drafted))


def test_generate_batch_and_errors(model, other):
    prompts = [_padded()[b, :p] for b, p in enumerate(PLENS)]
    base = model.generate_batch(prompts, NEW, temperature=0)
    got = model.generate_batch(prompts, NEW, temperature=0.8, top_k=1, sampler="native", draft=other, draft_k=3,
                               generator=_gen())
    assert all(torch.equal(a, b) for a, b in zip(got, base))
    idx = _padded()[:, :5]
    with pytest.raises(ValueError, match="temperature.*native"):
        model.generate(idx, NEW, temperature=0.8, draft=other)  # the default sampler has no verification
    with pytest.raises(ValueError, match="draft_k"):
        model.generate(idx, NEW, temperature=0.8, sampler="native", draft=other, draft_k=16)


def test_cli_passes_the_sampling_settings_to_a_draft_model():
    from replicann_amd.training import generate_main
    kw = ["--model", "gpt2-tiny", "--draft-model", "gpt2-tiny", "--device", "cpu", "--new", "6", "--prompt", "1,2,3",
          "--model-kwargs", '{"n_layer": 1, "n_embd": 64, "n_head": 2, "block_size": 32}']
    sampled = generate_main(kw + ["--temperature", "0.8", "--top-k", "50", "--sampler", "native"])
    assert len(sampled["tokens"][0]) == 6 and sampled["rounds"] >= 1 and sampled["drafted"][0] >= 4
    with pytest.raises(ValueError, match="native"):
        generate_main(kw + ["--temperature", "0.8", "--top-k", "50"])
