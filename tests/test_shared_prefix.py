"""n samples per prompt over one shared prompt KV cache, CPU tier: the composed path of
``ops.attention_decode_prefix`` in fp32 against the row-by-row reference (tests/prefix_cases.py), the buffers after
a call, and ``generate(num_samples=n)`` on a 2-layer fp32 model.

Bounds: the op within 1e-5 (allclose) of the fp32 reference and the model's logits within 1e-4 absolute of the plain
ragged cache run on the repeated prompts — the bounds tests/test_generate_ragged.py uses for the same comparisons
(same math, another summation order)."""

import pytest
import torch

import prefix_cases as C
from replicann_amd import ops
from replicann_amd.models.decoding import KVCache
from replicann_amd.models.gpt2 import GPT2, GPT2Config

H, D, P, L = 2, 64, 16, 8
PLENS = [20, 13]
N, NEW = 3, 12


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("G", [1, 3])
def test_op_matches_reference_and_leaves_the_buffers(G, n, index_dtype):
    """prefix_len in {0, 1, 7, P} x pos in {0, 3, L-1, L}: every pair, the pos values cycling over the batch rows."""
    for i, plen in enumerate((0, 1, 7, P)):
        for j in range(4):
            pos = [(0, 3, L - 1, L)[(b + j) % 4] for b in range(G * n)]
            plens = [(0, 1, 7, P)[(i + g) % 4] for g in range(G)] if j == 3 else [plen] * G
            out, ref, _ = C.run_case(ops.attention_decode_prefix, G, n, H, D, P, L, plens, pos, torch.float32, "cpu",
                                     index_dtype, seed=10 * i + j)
            assert torch.allclose(out, ref, atol=1e-5, rtol=1e-5), (plens, pos, (out - ref).abs().max().item())


def test_op_clamps_lengths_and_takes_other_head_sizes():
    out, ref, (qkv, before) = C.run_case(ops.attention_decode_prefix, 2, 2, 3, 16, P, L, [5000, -3], [L + 7, -1, 2, 5000],
                                         torch.float32, "cpu")
    assert torch.allclose(out, ref, atol=1e-5, rtol=1e-5)
    same, _, _ = C.run_case(ops.attention_decode_prefix, 2, 2, 3, 16, P, L, [P, 0], [L, 0, 2, L], torch.float32, "cpu")
    assert torch.equal(out, same)


def test_op_single_key_is_the_value_row():
    qkv, prefix, kv = C.make(1, 2, H, D, P, L, [0], [0, 0], torch.float32, "cpu")
    z = torch.zeros(2, dtype=torch.long)
    out = ops.attention_decode_prefix(qkv, prefix, z[:1], kv, z)
    assert torch.equal(out, qkv[:, :, 2])  # the softmax over one key is 1


def test_op_rejects_bad_arguments():
    qkv, prefix, kv = C.make(2, 2, H, D, P, L, [3, 3], [1] * 4, torch.float32, "cpu")
    plen, pos = torch.tensor([3, 3]), torch.ones(4, dtype=torch.long)
    ops.attention_decode_prefix(qkv, prefix, plen, kv, pos)
    bad = [
        (qkv[:, 0], prefix, plen, kv, pos),  # rank
        (qkv[:3], prefix, plen, kv[:3], pos[:3]),  # B not a multiple of G
        (qkv, prefix[..., :32], plen, kv, pos),  # D
        (qkv, prefix[:, :, :, :1], plen, kv, pos),  # H
        (qkv, prefix, plen, kv[:2], pos),  # tail batch
        (qkv, prefix, plen.float(), kv, pos),  # dtypes
        (qkv, prefix, plen, kv, pos.float()),
        (qkv, prefix.double(), plen, kv, pos),
        (qkv, prefix, plen[:1], kv, pos),  # counts
        (qkv, prefix, plen, kv, pos[:2]),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.attention_decode_prefix(*args)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.attention_decode_prefix(qkv.clone().requires_grad_(), prefix, plen, kv, pos)


# ------------------------------------------------------------------------------------------------
# the cache and generate
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GPT2(GPT2Config.tiny(n_embd=128, n_head=2, n_layer=2, block_size=128)).eval()


def _prompts():
    idx = torch.randint(0, 1000, (len(PLENS), max(PLENS)), generator=torch.Generator().manual_seed(1))
    pad = torch.arange(max(PLENS)).unsqueeze(0) >= torch.tensor(PLENS).unsqueeze(1)
    return idx.masked_fill(pad, 0)


def test_teacher_forced_logits_match_the_plain_ragged_cache(model):
    idx = _prompts()
    forced = torch.randint(0, 1000, (len(PLENS) * N, NEW), generator=torch.Generator().manual_seed(2))
    shared, plain = KVCache(2, 32, samples=N, tail_len=16), KVCache(2, 32)
    a = model.decode_step(idx, shared, lens=PLENS)
    b = model.decode_step(idx.repeat_interleave(N, 0), plain, lens=[p for p in PLENS for _ in range(N)])
    assert a.shape == (2, model.config.vocab_size)
    assert (a.repeat_interleave(N, 0) - b).abs().max().item() < 1e-4
    assert shared.per_seq and shared.prefix_len.tolist() == PLENS and shared.pos_t.tolist() == [0] * 6
    assert shared.prefix[0].shape == (2, 32, 2, 2, 64) and shared.kv[0].shape == (6, 16, 2, 2, 64)
    for t in range(NEW):
        a, b = model.decode_step(forced[:, t:t + 1], shared), model.decode_step(forced[:, t:t + 1], plain)
        err = (a - b).abs().max().item()
        assert err < 1e-4, (t, err)
    assert shared.pos_t.tolist() == [NEW] * 6 and shared.pos == NEW
    # the prompts' rows were written by the prefill alone
    for layer in range(2):
        for g, p in enumerate(PLENS):
            assert torch.equal(shared.prefix[layer][g, :p], plain.kv[layer][g * N, :p])
    # the tail is full at 16 rows
    for t in range(4):
        model.decode_step(forced[:, :1], shared)
    with pytest.raises(ValueError, match="full"):
        model.decode_step(forced[:, :1], shared)
    # device tensors survive reset(): a captured step reads them by address
    keep = (shared.prefix_len.data_ptr(), shared.pos_t.data_ptr(), shared.kv[0].data_ptr(), shared.prefix[0].data_ptr())
    shared.reset()
    model.decode_step(idx, shared, lens=PLENS)
    assert keep == (shared.prefix_len.data_ptr(), shared.pos_t.data_ptr(), shared.kv[0].data_ptr(),
                    shared.prefix[0].data_ptr())
    assert shared.pos_t.tolist() == [0] * 6


def test_generate_num_samples_greedy_rows_are_the_plain_run(model):
    """Greedy sampling makes every sample of a prompt the plain ragged run's row."""
    idx = _prompts()
    want, wl = model.generate(idx, NEW, prompt_lens=PLENS, temperature=0, graph=False)
    got, gl = model.generate(idx, NEW, prompt_lens=PLENS, temperature=0, graph=False, num_samples=N)
    assert got.shape == (6, max(PLENS) + NEW) and gl.tolist() == [p + NEW for p in PLENS for _ in range(N)]
    for b in range(6):
        assert torch.equal(got[b], want[b // N]), b


def test_generate_num_samples_uniform_and_sampled(model):
    idx = _prompts()[:, :13]
    out = model.generate(idx, NEW, temperature=1.0, top_k=50, generator=torch.Generator().manual_seed(3), graph=False,
                         num_samples=N)
    assert out.shape == (6, 13 + NEW) and torch.equal(out[:, :13], idx.repeat_interleave(N, 0))
    assert not torch.equal(out[0], out[1]) or not torch.equal(out[0], out[2])  # each sample draws its own tokens
    again = model.generate(idx, NEW, temperature=1.0, top_k=50, generator=torch.Generator().manual_seed(3), graph=False,
                           num_samples=N)
    assert torch.equal(out, again)
    nat = model.generate(idx, NEW, temperature=1.0, top_k=50, generator=torch.Generator().manual_seed(3), graph=False,
                         num_samples=N, sampler="native")
    assert nat.shape == out.shape


def test_eos_stops_one_sample_and_the_others_run_on(model):
    idx = _prompts()
    gen = lambda **kw: model.generate(idx, NEW, prompt_lens=PLENS, temperature=1.0, top_k=20, graph=False,  # noqa: E731
                                      generator=torch.Generator().manual_seed(5), num_samples=N, **kw)
    free, fl = gen()
    row = 1
    eos = int(free[row, PLENS[0] + 2])  # what sample 1 of prompt 0 emits at its third step
    stops = [free[b, fl[b] - NEW: fl[b]].tolist() for b in range(6)]
    tokens, lens = gen(eos_token_id=eos, pad_token_id=999)
    assert int(lens[row]) <= PLENS[0] + 3
    assert max(int(lens[0]), int(lens[2])) > int(lens[row])  # the other samples of its prompt run on
    for b in range(6):  # the draws do not depend on the other rows: every row is the free run's up to its own EOS
        p = PLENS[b // N]
        k = stops[b].index(eos) + 1 if eos in stops[b] else NEW
        assert int(lens[b]) == p + k, b
        assert torch.equal(tokens[b, :p + k], free[b, :p + k]) and bool((tokens[b, p + k:] == 999).all())


def test_num_samples_1_is_the_call_without_it(model):
    idx = _prompts()
    for kw in (dict(), dict(prompt_lens=PLENS), dict(prompt_lens=PLENS, eos_token_id=5)):
        a = model.generate(idx, NEW, temperature=0, graph=False, **kw)
        b = model.generate(idx, NEW, temperature=0, graph=False, num_samples=1, **kw)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else torch.equal(a, b)
    assert KVCache(2, 32, samples=1).shared is False


def test_generate_batch_returns_n_rows_per_prompt(model):
    prompts = [_prompts()[b, :p] for b, p in enumerate(PLENS)]
    rows = model.generate_batch(prompts, NEW, temperature=0, graph=False, num_samples=N)
    plain = model.generate_batch(prompts, NEW, temperature=0, graph=False)
    assert len(rows) == 6 and all(torch.equal(r, plain[b // N]) for b, r in enumerate(rows))


def test_cli_num_samples_groups_by_prompt(model, tmp_path, capsys):
    import json

    from replicann_amd import cli
    from replicann_amd.utils.checkpoint import save_checkpoint
    ck = tmp_path / "ck.pt"
    save_checkpoint(str(ck), model, step=1)
    idx = _prompts()
    base = ["generate", "--model", "gpt2-tiny", "--model-kwargs", json.dumps({"n_head": 2}), "--checkpoint", str(ck),
            "--new", str(NEW), "--temperature", "0", "--device", "cpu", "--num-samples", str(N)]
    argv = list(base)
    for b, p in enumerate(PLENS):
        argv += ["--prompt", ",".join(map(str, idx[b, :p].tolist()))]
    cli.main(argv)
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want, _ = model.generate(idx, NEW, prompt_lens=PLENS, temperature=0, graph=False)
    assert res["prompt_lens"] == PLENS and res["lengths"] == [[p + NEW] * N for p in PLENS]
    for g, p in enumerate(PLENS):
        assert res["tokens"][g] == [want[g, p:p + NEW].tolist()] * N
    cli.main(base + ["--prompt", ",".join(map(str, idx[1, :13].tolist()))])  # one prompt: the uniform path
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["tokens"] == [[want[1, 13:13 + NEW].tolist()] * N]


def test_errors(model):
    idx = _prompts()
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="num_samples"):
            model.generate(idx, 4, num_samples=bad)
    with pytest.raises(ValueError, match="draft"):
        model.generate(idx, 4, temperature=0, num_samples=2, draft=model)
    with pytest.raises(ValueError, match="kv_dtype"):
        model.generate(idx, 4, temperature=0, num_samples=2, kv_dtype="fp8")
    with pytest.raises(ValueError, match="fp8"):
        KVCache(2, 32, "fp8", samples=2)
    for bad in (0, 1.5, None):
        with pytest.raises(ValueError, match="samples"):
            KVCache(2, 32, samples=bad)
    cache = KVCache(2, 32, samples=2, tail_len=8)
    model.decode_step(idx, cache, lens=PLENS)
    with pytest.raises(ValueError, match="window"):
        model.decode_window(torch.zeros(4, 2, dtype=torch.long), cache)
    with pytest.raises(ValueError, match="window"):
        cache.window(0, torch.zeros(4, 2, 3, 2, 64))
    with pytest.raises(ValueError):  # one token per row and step
        model.decode_step(torch.zeros(4, 2, dtype=torch.long), cache)
