"""Speculative decoding on the CPU (fp32, one reference arithmetic): ``decoding.accept`` on hand-written
cases, ``ops.attention_window`` (composed path) against ``attention_reference`` per query, the
teacher-forced window step with partial ``advance`` over stale rows, and ``generate(draft=...)``
token for token against plain greedy generation."""

import pytest
import torch

import replicann_amd as R
from replicann_amd import ops
from replicann_amd.models.decoding import KVCache, accept

PLENS = [5, 20, 13]
NEW = 12


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


# ------------------------------------------------------------------ accept
def _accept(drafts, greedy, **kw):
    c, t, a = accept(torch.tensor(drafts), torch.tensor(greedy), **kw)
    return c.tolist(), t.tolist(), a.tolist()


def test_accept_prefix_lengths():
    # a = 0 (first draft wrong), a in the middle, a = K
    drafts = [[9, 2, 3], [1, 2, 9], [1, 2, 3]]
    greedy = [[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3, 4]]
    count, toks, a = _accept(drafts, greedy, pad=-1)
    assert a == [0, 2, 3] and count == [1, 3, 4]
    assert toks == [[1, -1, -1, -1], [1, 2, 3, -1], [1, 2, 3, 4]]


def test_accept_a_later_match_after_a_mismatch_does_not_count():
    count, toks, a = _accept([[1, 9, 3]], [[1, 2, 3, 4]], pad=0)
    assert a == [1] and count == [2] and toks == [[1, 2, 0, 0]]


def test_accept_eos_cuts_and_is_kept():
    # EOS (7) inside the accepted run; EOS as the target's own token; EOS only past the committed ones
    drafts = [[1, 7, 3], [1, 9, 3], [9, 7, 3]]
    greedy = [[1, 7, 3, 4], [1, 7, 3, 4], [1, 7, 3, 4]]
    count, toks, a = _accept(drafts, greedy, eos=7, pad=0)
    assert a == [3, 1, 0] and count == [2, 2, 1]
    assert toks == [[1, 7, 0, 0], [1, 7, 0, 0], [1, 0, 0, 0]]


def test_accept_budget_and_finished_rows():
    drafts = [[1, 2, 3], [1, 2, 3], [1, 2, 3]]
    greedy = [[1, 2, 3, 4]] * 3
    count, toks, a = _accept(drafts, greedy, budget=torch.tensor([2, 9, 0]), finished=torch.tensor([False, True, False]),
                             pad=5)
    assert a == [3, 3, 3] and count == [2, 0, 0]
    assert toks == [[1, 2, 5, 5], [5, 5, 5, 5], [5, 5, 5, 5]]


# ------------------------------------------------------------------ ops.attention_window (composed path)
def _window_case(B, T, H, D, L, pos, seed=0):
    torch.manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, D)
    kv = torch.randn(B, L, 2, H, D)
    for b, p in enumerate(pos):
        kv[b, max(min(p, L), 0):] = float("nan")  # never read: stale / unwritten rows
    return qkv, kv


def _check_window(qkv, kv, pos, out, before):
    B, T, _, H, D = qkv.shape
    L = kv.shape[1]
    assert bool(torch.isfinite(out).all())
    for b, p in enumerate(pos):
        p = max(min(p, L), 0)
        for i in range(T):  # the query's own keys: cache rows < pos, window rows <= i
            k = torch.cat([before[b, :p, 0], qkv[b, : i + 1, 1]]).unsqueeze(0)
            v = torch.cat([before[b, :p, 1], qkv[b, : i + 1, 2]]).unsqueeze(0)
            ref = ops.attention_reference(qkv[b: b + 1, i: i + 1, 0], k, v, D ** -0.5)
            torch.testing.assert_close(out[b: b + 1, i: i + 1], ref, rtol=1e-4, atol=1e-5)
        want = before[b].clone()
        n = max(min(T, L - p), 0)
        want[p: p + n] = qkv[b, :n, 1:3]
        # bitwise (NaN rows included): exactly the in-range window rows replaced
        assert torch.equal(kv[b].view(torch.int32), want.view(torch.int32)), b


@pytest.mark.parametrize("T", [1, 5, 20])
def test_attention_window_cpu(T):
    pos = [0, 1, 17, 40]
    qkv, kv = _window_case(4, T, 2, 32, 64, pos)
    before = kv.clone()
    out = ops.attention_window(qkv, kv, torch.tensor(pos))
    assert out.shape == (4, T, 2, 32)
    _check_window(qkv, kv, pos, out, before)


def test_attention_window_cpu_clamps_and_skips_rows_that_do_not_fit():
    L, T = 40, 5
    pos = [L - 2, L, -1, 1 << 40]
    qkv, kv = _window_case(4, T, 2, 64, L, pos)
    before = kv.clone()
    out = ops.attention_window(qkv, kv, torch.tensor(pos))
    _check_window(qkv, kv, pos, out, before)
    changed = (kv.view(torch.int32) != before.view(torch.int32)).flatten(2).any(2)
    assert changed[0].nonzero().flatten().tolist() == [L - 2, L - 1]  # two rows and nothing else
    assert not bool(changed[1].any()) and not bool(changed[3].any())
    assert changed[2].nonzero().flatten().tolist() == list(range(T))


def test_attention_window_int32_pos_and_bad_pos():
    qkv, kv = _window_case(2, 3, 2, 32, 16, [4, 9])
    kv2 = kv.clone()
    a = ops.attention_window(qkv, kv, torch.tensor([4, 9]))
    b = ops.attention_window(qkv, kv2, torch.tensor([4, 9], dtype=torch.int32))
    assert torch.equal(a, b) and torch.equal(kv.view(torch.int32), kv2.view(torch.int32))
    with pytest.raises(ValueError):
        ops.attention_window(qkv, kv, torch.tensor([4]))
    with pytest.raises(ValueError):
        ops.attention_window(qkv, kv, torch.tensor([4.0, 9.0]))


# ------------------------------------------------------------------ the window step, teacher-forced
def test_decode_window_teacher_forced(model):
    """Windows and one-token steps over one cache, with partial advances that leave stale rows behind:
    every output is the full forward's argmax at the row's own position of the TRUE sequence."""
    g = torch.Generator().manual_seed(3)
    total = 48
    seq = torch.randint(0, 1000, (3, total), generator=g)  # row b's true sequence
    with torch.no_grad():
        full = model(seq).argmax(-1)  # (3, total): the greedy token after each position
    cache = KVCache(2, 64)
    idx = torch.stack([torch.cat([seq[b, :p], seq.new_zeros(max(PLENS) - p)]) for b, p in enumerate(PLENS)])
    model.decode_step(idx, cache, lens=PLENS)
    at = list(PLENS)  # each row's position

    def window(T, counts, wrong_after=None):
        toks = torch.stack([seq[b, at[b]: at[b] + T] for b in range(3)]).clone()
        if wrong_after is not None:  # what will not be committed is junk: it must leave no trace
            for b, c in enumerate(counts):
                toks[b, c:] = 999
        before = cache.pos_t.clone()
        ids = model.decode_window(toks, cache)
        assert torch.equal(cache.pos_t, before)  # the window step does not move the position
        for b, c in enumerate(counts):
            assert ids[b, :c].tolist() == full[b, at[b]: at[b] + c].tolist(), b
        cache.advance(torch.tensor(counts))
        for b, c in enumerate(counts):
            at[b] += c
        assert cache.pos_t.tolist() == at and cache.lens.tolist() == [a + 1 for a in at]

    window(5, [5, 5, 5])
    window(5, [1, 3, 0], wrong_after=True)  # partial: rows past the count hold junk keys / values
    logits = model.decode_step(torch.stack([seq[b, at[b]] for b in range(3)]).view(3, 1), cache)  # a one-token step
    assert logits.argmax(-1).tolist() == [int(full[b, at[b]]) for b in range(3)]
    at = [a + 1 for a in at]
    window(3, [2, 1, 3], wrong_after=True)
    window(1, [1, 1, 1])
    window(8, [8, 4, 6], wrong_after=True)
    cache.active.copy_(torch.tensor([1, 0, 1]))  # a finished row does not advance
    before = list(at)
    cache.advance(torch.tensor([0, 2, 0]))
    assert cache.pos_t.tolist() == before


def test_window_entry_points_need_per_sequence_mode(model):
    cache = KVCache(2, 64)
    model.decode_step(torch.zeros(2, 4, dtype=torch.long), cache)  # host mode
    with pytest.raises(ValueError):
        model.decode_window(torch.zeros(2, 3, dtype=torch.long), cache)
    with pytest.raises(ValueError):
        cache.advance(torch.tensor([1, 1]))
    with pytest.raises(ValueError):
        cache.set_rows(torch.tensor([1, 1]))


def test_per_sequence_decode_step_still_takes_one_token(model):
    cache = KVCache(2, 64)
    model.decode_step(_padded(), cache, lens=PLENS)
    with pytest.raises(ValueError, match="one token per row"):
        model.decode_step(torch.zeros(3, 2, dtype=torch.long), cache)
    with pytest.raises(ValueError, match="one token per step"):
        cache.update(0, torch.zeros(3, 2, 2, 4, 32))


# ------------------------------------------------------------------ generate(draft=...)
@pytest.mark.parametrize("k", [1, 4])
def test_generate_with_the_same_model_as_draft_accepts_everything(model, k):
    idx = _padded()[:, :5]
    base = model.generate(idx, NEW, temperature=0)
    stats = {}
    out = model.generate(idx, NEW, temperature=0, draft=model, draft_k=k, stats=stats)
    assert torch.is_tensor(out) and torch.equal(out, base)
    # the first token comes from the prefill, then every round commits k + 1 until the budget cuts the last
    assert stats["rounds"] == -(-(NEW - 1) // (k + 1))
    assert stats["drafted"].tolist() == [k * stats["rounds"]] * 3
    assert stats["accepted"].tolist() == stats["drafted"].tolist()


@pytest.mark.parametrize("k", [1, 4])
def test_generate_with_another_draft_equals_plain_greedy(model, other, k):
    idx = _padded()[:, :5]
    base = model.generate(idx, NEW, temperature=0)
    stats = {}
    out = model.generate(idx, NEW, temperature=0, draft=other, draft_k=k, stats=stats)
    assert torch.equal(out, base)
    assert all(0 <= a <= d for a, d in zip(stats["accepted"].tolist(), stats["drafted"].tolist()))
    assert (NEW - 1 + k) // (k + 1) <= stats["rounds"] <= NEW - 1


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("which", ["same", "other"])
def test_generate_ragged_with_eos_equals_plain_greedy(model, other, k, which):
    draft = model if which == "same" else other
    base, blens = model.generate(_padded(), NEW, temperature=0, prompt_lens=PLENS)
    tokens, lens = model.generate(_padded(junk=True), NEW, temperature=0, prompt_lens=PLENS, draft=draft, draft_k=k)
    assert torch.equal(tokens, base) and torch.equal(lens, blens)
    eos = int(base[1, PLENS[1] + 3])  # an EOS taken from the base run: row 1 stops after 4 tokens at the latest
    want, wlens = model.generate(_padded(), NEW, temperature=0, prompt_lens=PLENS, eos_token_id=eos, pad_token_id=0)
    assert int(wlens[1]) <= PLENS[1] + 4
    got, glens = model.generate(_padded(), NEW, temperature=0, prompt_lens=PLENS, eos_token_id=eos, pad_token_id=0,
                                draft=draft, draft_k=k)
    assert torch.equal(glens, wlens) and torch.equal(got, want)


def test_generate_batch_takes_a_draft(model, other):
    prompts = [_padded()[b, :p] for b, p in enumerate(PLENS)]
    base = model.generate_batch(prompts, NEW, temperature=0)
    got = model.generate_batch(prompts, NEW, temperature=0, draft=other, draft_k=3)
    assert all(torch.equal(a, b) for a, b in zip(got, base))


def test_generate_draft_errors(model, other):
    idx = _padded()[:, :5]
    with pytest.raises(ValueError, match="temperature"):
        model.generate(idx, NEW, draft=other)  # the default temperature samples
    for k in (0, 16):
        with pytest.raises(ValueError, match="draft_k"):
            model.generate(idx, NEW, temperature=0, draft=other, draft_k=k)
    with pytest.raises(ValueError, match="vocab_size"):
        model.generate(idx, NEW, temperature=0, draft=_model(vocab_size=900))
    with pytest.raises(ValueError, match="dtype"):
        model.generate(idx, NEW, temperature=0, draft=_model().double())
    with pytest.raises(ValueError, match="device"):
        model.generate(idx, NEW, temperature=0, draft=_model().to("meta"))
    # 5 + 119 + 4 = 128 fits; one more token does not (the window writes draft_k rows past the last token)
    with pytest.raises(ValueError, match="target model's block_size"):
        model.generate(idx, 120, temperature=0, draft=other, draft_k=4)
    with pytest.raises(ValueError, match="draft model's block_size"):
        model.generate(idx, 60, temperature=0, draft=_model(block_size=64), draft_k=4)
