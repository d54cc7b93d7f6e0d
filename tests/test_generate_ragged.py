"""Batched generation over prompts of different lengths with an EOS stop, on the CPU path (fp32):
the ops' ``lens`` / per-row ``pos`` fallbacks, the per-sequence KV cache mode, ``GPT2.generate`` with
``prompt_lens`` / ``eos_token_id``, ``generate_batch`` and the CLI.

Greedy criterion (that of tests/test_generate_gpu.py, with an fp32 margin): the chosen token's logit
is within 1e-4 · max|logit| of the maximum of the full forward of the row's own unpadded prefix —
the cached step and the full forward are the same fp32 math in another order, whose difference on
this model is ~1e-6 relative; 1e-4 leaves two orders of magnitude and still separates any token
that is not a (near-)tie for the top."""

import json

import pytest
import torch

from replicann_amd import ops
from replicann_amd.models import GPT2, GPT2Config
from replicann_amd.models import gpt2 as G
from replicann_amd.models.blocks import KVCache

PLENS = [5, 20, 13]
NEW = 12


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GPT2(GPT2Config.tiny(n_embd=128, n_head=2, n_layer=2, block_size=128)).eval()


def _padded(fill_seed=None):
    """(3, 20) right-padded prompts of PLENS; the padding is 0, or random valid ids."""
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 1000, (len(PLENS), max(PLENS)), generator=g)
    pad = torch.arange(max(PLENS)).unsqueeze(0) >= torch.tensor(PLENS).unsqueeze(1)
    if fill_seed is None:
        return idx.masked_fill(pad, 0)
    junk = torch.randint(0, 1000, idx.shape, generator=torch.Generator().manual_seed(fill_seed))
    return torch.where(pad, junk, idx)


@pytest.fixture(scope="module")
def no_eos(model):
    """The ragged greedy run without EOS, computed once: (tokens, lens)."""
    tokens, lens = model.generate(_padded(), NEW, prompt_lens=PLENS, temperature=0, graph=False)
    return tokens.clone(), lens.clone()


def test_attention_decode_lens_fallback():
    torch.manual_seed(0)
    B, H, Tk, D = 4, 2, 19, 16
    q, k, v = torch.randn(B, 1, H, D), torch.randn(B, Tk, H, D), torch.randn(B, Tk, H, D)
    for dtype in (torch.int32, torch.int64):
        lens = torch.tensor([1, 7, 19, 12], dtype=dtype)
        o = ops.attention_decode(q, k, v, lens=lens)
        for b, n in enumerate(lens.tolist()):
            ref = ops.attention_reference(q[b:b + 1], k[b:b + 1, :n], v[b:b + 1, :n], D ** -0.5)
            assert torch.allclose(o[b:b + 1], ref, atol=1e-5, rtol=1e-5), (b, n)
    o = ops.attention_decode(q, k, v, lens=torch.tensor([0, 3, 0, 19]))
    assert bool((o[0] == 0).all()) and bool((o[2] == 0).all()) and bool(torch.isfinite(o).all())
    with pytest.raises(ValueError):
        ops.attention_decode(q, k, v, torch.zeros(Tk), lens=lens)
    with pytest.raises(ValueError):
        ops.attention_decode(q, k, v, lens=torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError):
        ops.attention_decode(q, k, v, lens=torch.tensor([1.0, 2.0, 3.0, 4.0]))


def test_linear_kv_append_per_row_fallback():
    torch.manual_seed(0)
    B, H, D, L = 5, 2, 8, 40
    E = H * D
    x, w, bias = torch.randn(B, 1, E), torch.randn(3 * E, E), torch.randn(3 * E)
    pos = torch.tensor([0, 39, 17, 17, 3])
    before = torch.randn(B, L, 2, H, D)
    kv = before.clone()
    with torch.no_grad():
        y = ops.linear_kv_append(x, w, bias, kv, pos)
        y1 = ops.linear_kv_append(x, w, bias, before.clone(), torch.tensor([7]))
    assert torch.equal(y, y1)  # the one-element call: same y
    want = before.clone()
    for b, p in enumerate(pos.tolist()):
        want[b, p] = y[b, 0, E:].view(2, H, D)
    assert torch.equal(kv, want)  # row pos[b] of batch row b and nothing else
    # a position outside [0, L) appends nothing
    kv2 = before.clone()
    with torch.no_grad():
        ops.linear_kv_append(x, w, bias, kv2, torch.tensor([0, 40, -1, 17, 3]))
    want[1, 39], want[2, 17] = before[1, 39], before[2, 17]
    assert torch.equal(kv2, want)
    with pytest.raises(ValueError):
        ops.linear_kv_append(x, w, bias, kv2, torch.tensor([0, 1]))


def _assert_greedy(model, tokens, lens, margin=1e-4):
    for b, p in enumerate(PLENS):
        row = tokens[b, : int(lens[b])]
        with torch.no_grad():
            full = model(row.unsqueeze(0))[0]  # the row's own unpadded sequence
        for t in range(p, int(lens[b])):
            lg = full[t - 1]
            assert lg[row[t]] >= lg.max() - margin * lg.abs().max(), (b, t)


def test_ragged_greedy_matches_full_forward(model, no_eos):
    tokens, lens = no_eos
    idx = _padded()
    assert lens.tolist() == [p + NEW for p in PLENS] and tokens.shape == (3, max(PLENS) + NEW)
    for b, p in enumerate(PLENS):
        assert torch.equal(tokens[b, :p], idx[b, :p])
        assert bool((tokens[b, p + NEW:] == 0).all())  # right-padded with the pad id
    _assert_greedy(model, tokens, lens)


def test_decode_step_lens_per_sequence_cache(model):
    """Teacher-forced: the ragged prefill's and every later step's logits are the full forward's at
    each row's own position; the cache advances every row from its own length."""
    g = torch.Generator().manual_seed(2)
    seqs = [torch.randint(0, 1000, (p + 6,), generator=g) for p in PLENS]
    idx = torch.zeros(3, max(PLENS), dtype=torch.long)
    for b, p in enumerate(PLENS):
        idx[b, :p] = seqs[b][:p]
    with torch.no_grad():
        full = [model(s.unsqueeze(0))[0] for s in seqs]
    cache = KVCache(model.config.n_layer, max(PLENS) + 6)
    lg = model.decode_step(idx, cache, lens=PLENS)
    assert cache.per_seq and cache.pos_t.tolist() == PLENS and cache.lens.tolist() == [p + 1 for p in PLENS]
    for t in range(6):
        for b, p in enumerate(PLENS):
            assert (lg[b] - full[b][p + t - 1]).abs().max().item() < 1e-4, (b, t)
        tok = torch.stack([seqs[b][p + t] for b, p in enumerate(PLENS)]).view(3, 1)
        lg = model.decode_step(tok, cache)
    assert cache.pos_t.tolist() == [p + 6 for p in PLENS]
    with pytest.raises(ValueError):  # the longest row has reached the cache length
        model.decode_step(tok, cache)
    with pytest.raises(ValueError):
        model.decode_step(idx, KVCache(model.config.n_layer, 32), lens=[5, 21, 13])
    with pytest.raises(ValueError):
        model.decode_step(idx, KVCache(model.config.n_layer, 32), lens=[0, 20, 13])


def test_padding_content_is_ignored(model, no_eos):
    tokens, lens = model.generate(_padded(fill_seed=7), NEW, prompt_lens=PLENS, temperature=0, graph=False)
    assert torch.equal(tokens, no_eos[0]) and torch.equal(lens, no_eos[1])


def test_eos_stops_rows(model, no_eos):
    base, _ = no_eos
    eos = int(base[0, PLENS[0] + 3])  # the token row 0 produced at its 4th step
    tokens, lens = model.generate(_padded(), NEW, prompt_lens=PLENS, eos_token_id=eos, temperature=0, graph=False)
    assert tokens.shape[1] == int(lens.max())
    for b, p in enumerate(PLENS):
        gen = base[b, p: p + NEW].tolist()
        n = p + (gen.index(eos) + 1 if eos in gen else NEW)
        assert int(lens[b]) == n, b
        assert torch.equal(tokens[b, :n], base[b, :n])  # up to and including the first EOS
        assert bool((tokens[b, n:] == eos).all())  # pad (default: the EOS id) after that
    assert int(lens[0]) <= PLENS[0] + 4
    # an explicit pad id
    tp, lp = model.generate(_padded(), NEW, prompt_lens=PLENS, eos_token_id=eos, pad_token_id=999, temperature=0,
                            graph=False)
    assert torch.equal(lp, lens)
    for b in range(3):
        assert torch.equal(tp[b, : int(lp[b])], tokens[b, : int(lp[b])]) and bool((tp[b, int(lp[b]):] == 999).all())


def test_eos_batch1_returns_short_row_and_stops_early(model, no_eos, monkeypatch):
    base, _ = no_eos
    p = PLENS[0]
    eos = int(base[0, p + 3])
    first = base[0, p: p + NEW].tolist().index(eos)
    steps = []
    real = GPT2._device_position_step
    monkeypatch.setattr(GPT2, "_device_position_step", lambda self, tok, cache: (steps.append(1), real(self, tok, cache))[1])
    tokens, lens = model.generate(base[:1, :p], 40, eos_token_id=eos, temperature=0, graph=False)
    assert tokens.shape == (1, p + first + 1) and tokens.shape[1] < p + 40 and int(lens[0]) == p + first + 1
    assert torch.equal(tokens[0], base[0, : p + first + 1])
    # every row finished: the loop ends at the next DECODE_EOS_CHECK boundary, not after 40 steps
    assert len(steps) < G.DECODE_EOS_CHECK * (first // G.DECODE_EOS_CHECK + 1)


def test_uniform_call_unchanged(model):
    idx = _padded()
    out = model.generate(idx, 4, temperature=0, graph=False)
    assert torch.is_tensor(out) and out.shape == (3, 24)
    tokens, lens = model.generate(idx, 4, prompt_lens=[20, 20, 20], temperature=0, graph=False)
    assert torch.equal(tokens, out) and lens.tolist() == [24, 24, 24]


@pytest.mark.parametrize("plens,new", [([0, 20, 13], 4), ([5, 21, 13], 4), ([5, 20], 4), ([5, 20, 13], 109),
                                       ([-1, 20, 13], 4)])
def test_invalid_prompt_lens_and_capacity(model, plens, new):
    with pytest.raises(ValueError):
        model.generate(_padded(), new, prompt_lens=plens, temperature=0)  # 20 + 109 > block_size 128


def test_generate_batch(model, no_eos):
    idx = _padded()
    rows = model.generate_batch([idx[b, :p] for b, p in enumerate(PLENS)], NEW, temperature=0, graph=False)
    assert [r.numel() for r in rows] == [p + NEW for p in PLENS]
    for b, r in enumerate(rows):
        assert r.dim() == 1 and torch.equal(r, no_eos[0][b, : r.numel()])


def test_cli_ragged(model, no_eos, tmp_path, capsys):
    from replicann_amd import cli
    from replicann_amd.utils.checkpoint import save_checkpoint
    ck = tmp_path / "ck.pt"
    save_checkpoint(str(ck), model, step=1)
    base = no_eos[0]
    eos = int(base[0, PLENS[0] + 3])
    idx = _padded()
    argv = ["generate", "--model", "gpt2-tiny", "--model-kwargs", json.dumps({"n_head": 2}), "--checkpoint", str(ck),
            "--new", str(NEW), "--temperature", "0", "--device", "cpu", "--eos", str(eos)]
    for b in (0, 2):
        argv += ["--prompt", ",".join(map(str, idx[b, : PLENS[b]].tolist()))]
    cli.main(argv)
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(res["tokens"]) == 2 and res["prompt_lens"] == [PLENS[0], PLENS[2]]
    want, _ = model.generate(idx[[0, 2]], NEW, prompt_lens=[PLENS[0], PLENS[2]], eos_token_id=eos, temperature=0,
                             graph=False)
    for i, b in enumerate((0, 2)):
        n = res["lengths"][i]
        assert res["tokens"][i] == want[i, PLENS[b]: n].tolist()
    assert res["tokens"][0][-1] == eos and res["lengths"][0] == PLENS[0] + len(res["tokens"][0])
