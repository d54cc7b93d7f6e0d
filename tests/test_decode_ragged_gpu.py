"""Ragged decoding on the HIP kernels: the one-query attention with per-sequence lengths, the K|V
append at per-row positions, the per-sequence KV cache under ``decode_step`` (eager and captured)
and ``GPT2.generate(prompt_lens=..., eos_token_id=...)``.

Kernel shapes sit at the one-query kernel's own edges: the 32 key groups of P·V, the 64-lane wave,
the 256 threads (past which a thread takes a second key) and the 1024-key maximum.

Tolerances: 1e-2 relative L2 for the attention (the bound tests/test_ops_gpu.py uses for the same
arithmetic), 3e-2 on the logits of the 2-layer bf16 model (stated and derived in
tests/test_generate_gpu.py)."""

import copy

import pytest
import torch

from replicann_amd import ops

pytestmark = pytest.mark.gpu

PLENS = [5, 20, 13]
NEW = 12


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _model(cuda, n_head):
    import replicann_amd as R
    torch.manual_seed(0)
    m = R.GPT2(R.GPT2Config.tiny(n_embd=128, n_head=n_head, n_layer=2, block_size=128)).to(cuda)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m.eval()


def _fp32(m):
    return copy.deepcopy(m).float().cpu().eval()


def _padded(cuda, seed=1, junk=False):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 1000, (len(PLENS), max(PLENS)), generator=g)
    pad = torch.arange(max(PLENS)).unsqueeze(0) >= torch.tensor(PLENS).unsqueeze(1)
    fill = torch.randint(0, 1000, idx.shape, generator=g) if junk else torch.zeros_like(idx)
    return torch.where(pad, fill, idx).to(cuda)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_attention_decode_lens(cuda, dtype):
    torch.manual_seed(0)
    B, H, Tk = 8, 2, 1024
    lens = [1, 31, 33, 64, 255, 257, 1000, 1024]
    q = torch.randn(B, 1, 3, H, 64, device=cuda).bfloat16()[:, :, 0]
    buf = torch.randn(B, Tk, 2, H, 64, device=cuda).bfloat16()
    for b, n in enumerate(lens):
        buf[b, n:] = float("nan")  # every K and V row at or past lens[b]: never read
    k, v = buf[:, :, 0], buf[:, :, 1]
    lens_t = torch.tensor(lens, dtype=dtype, device=cuda)
    with torch.no_grad():
        o = ops.attention_decode(q, k, v, lens=lens_t)
        o2 = ops.attention_decode(q, k, v, lens=lens_t)
    assert o.shape == (B, 1, H, 64) and bool(torch.isfinite(o).all())
    for b, n in enumerate(lens):
        ref = ops.attention_reference(q[b:b + 1].float(), k[b:b + 1, :n].float(), v[b:b + 1, :n].float(), 64 ** -0.5)
        assert rel_err(o[b:b + 1], ref) < 1e-2, (b, n)
    assert torch.equal(o, o2)  # bitwise deterministic
    # a length past the view is clamped to it (row 7's view is fully written)
    with torch.no_grad():
        o3 = ops.attention_decode(q[7:], k[7:], v[7:], lens=torch.tensor([5000], dtype=dtype, device=cuda))
    assert torch.equal(o3, o[7:])


@pytest.mark.parametrize("Tk", [19, 129, 1024])
def test_attention_decode_lens_full_is_unmasked_kernel(cuda, Tk):
    torch.manual_seed(Tk)
    B, H = 8, 2
    q = torch.randn(B, 1, 3, H, 64, device=cuda).bfloat16()[:, :, 0]
    buf = torch.randn(B, 1024, 2, H, 64, device=cuda).bfloat16()
    k, v = buf[:, :Tk, 0], buf[:, :Tk, 1]
    with torch.no_grad():
        a = ops.attention_decode(q, k, v, lens=torch.full((B,), Tk, dtype=torch.int32, device=cuda))
        b = ops.attention_decode(q, k, v, None)
    assert torch.equal(a, b)


def test_attention_decode_lens_zero_and_checks(cuda):
    torch.manual_seed(0)
    B, H, Tk = 4, 2, 129
    q = torch.randn(B, 1, 3, H, 64, device=cuda).bfloat16()[:, :, 0]
    buf = torch.randn(B, Tk, 2, H, 64, device=cuda).bfloat16()
    k, v = buf[:, :, 0], buf[:, :, 1]
    lens = torch.tensor([0, 40, 0, 129], device=cuda)
    with torch.no_grad():
        o = ops.attention_decode(q, k, v, lens=lens)
        assert bool((o[0] == 0).all()) and bool((o[2] == 0).all())
        ref = ops.attention_reference(q[1:2].float(), k[1:2, :40].float(), v[1:2, :40].float(), 64 ** -0.5)
        assert rel_err(o[1:2], ref) < 1e-2
        with pytest.raises(ValueError):
            ops.attention_decode(q, k, v, torch.zeros(1, 1, Tk, device=cuda), lens=lens)
        with pytest.raises(ValueError):
            ops.attention_decode(q, k, v, lens=lens.cpu())
        with pytest.raises(RuntimeError):  # the binding's own checks
            torch.ops.replicann.attn_decode(q, k, v, None, 0.125, lens[:3])
        with pytest.raises(RuntimeError):
            torch.ops.replicann.attn_decode(q, k, v, None, 0.125, lens.float())
        with pytest.raises(RuntimeError):
            torch.ops.replicann.attn_decode(q, k, v, torch.zeros(Tk, device=cuda), 0.125, lens)


@pytest.mark.parametrize("B,H,pos", [(5, 2, [0, 39, 17, 17, 3]), (64, 12, [b % 40 for b in range(64)])])
def test_linear_kv_append_per_row(cuda, B, H, pos):
    torch.manual_seed(B + H)
    E, L = 64 * H, 40
    x = torch.randn(B, 1, E, device=cuda).bfloat16()
    w = (torch.randn(3 * E, E, device=cuda) * 0.05).bfloat16()
    bias = (torch.randn(3 * E, device=cuda) * 0.1).bfloat16()
    before = torch.randn(B, L, 2, H, 64, device=cuda).bfloat16()
    kv = before.clone()
    with torch.no_grad():
        y = ops.linear_kv_append(x, w, bias, kv, torch.tensor(pos, device=cuda))
        y1 = ops.linear_kv_append(x, w, bias, before.clone(), torch.tensor([17], device=cuda))
    assert torch.equal(y, y1)
    want = before.clone()
    for b, p in enumerate(pos):
        want[b, p] = y[b, 0, E:].view(2, H, 64)
    assert torch.equal(kv, want)  # kv[b, pos[b]] is y's K|V columns, every other row unchanged


def test_linear_kv_append_out_of_range_rows_skipped(cuda):
    torch.manual_seed(0)
    B, H, E, L = 5, 2, 128, 40
    x = torch.randn(B, 1, E, device=cuda).bfloat16()
    w = (torch.randn(3 * E, E, device=cuda) * 0.05).bfloat16()
    before = torch.randn(B, L, 2, H, 64, device=cuda).bfloat16()
    kv = before.clone()
    with torch.no_grad():
        y = ops.linear_kv_append(x, w, None, kv, torch.tensor([0, 40, -1, 1 << 40, 39], device=cuda))
    want = before.clone()
    want[0, 0], want[4, 39] = y[0, 0, E:].view(2, H, 64), y[4, 0, E:].view(2, H, 64)
    assert torch.equal(kv, want)


# ------------------------------------------------------------------ model
@pytest.mark.parametrize("n_head", [2, 4])
def test_decode_step_ragged_eager_and_captured(cuda, n_head):
    """Teacher-forced ragged decoding (n_head 2: the lengths kernel; 4: the bias fallback), eager and
    captured / replayed, each row against the fp32 forward of its own sequence at its own position."""
    from replicann_amd.models.blocks import KVCache
    m = _model(cuda, n_head)
    ref = _fp32(m)
    g = torch.Generator().manual_seed(3)
    seqs = [torch.randint(0, 1000, (p + NEW,), generator=g) for p in PLENS]
    with torch.no_grad():
        full = [ref(s.unsqueeze(0))[0] for s in seqs]
    idx = torch.zeros(3, max(PLENS), dtype=torch.long)
    for b, p in enumerate(PLENS):
        idx[b, :p] = seqs[b][:p]
    idx = idx.to(cuda)
    toks = [torch.stack([seqs[b][p + t] for b, p in enumerate(PLENS)]).view(3, 1).to(cuda) for t in range(NEW)]

    def check(lg, t):
        for b, p in enumerate(PLENS):
            assert rel_err(lg[b], full[b][p + t - 1]) < 3e-2, (b, t)

    eager = KVCache(m.config.n_layer, 64)
    lg = m.decode_step(idx, eager, lens=PLENS)
    for t in range(NEW):
        check(lg, t)
        lg = m.decode_step(toks[t], eager)
    assert eager.pos_t.tolist() == [p + NEW for p in PLENS]

    cap = KVCache(m.config.n_layer, 64)
    lg = m.decode_step(idx, cap, lens=PLENS)
    graph, tok, out = m._capture_decode(cap, 3)
    assert cap.pos_t.tolist() == PLENS  # capture leaves the cache where the prefill did
    for t in range(NEW):
        check(lg, t)
        tok.copy_(toks[t])
        graph.replay()
        lg = out
    torch.cuda.synchronize()
    assert cap.pos_t.tolist() == [p + NEW for p in PLENS]
    assert cap.lens.tolist() == [p + NEW + 1 for p in PLENS]


def _assert_greedy(ref, tokens, lens, margin=3e-2):
    for b, p in enumerate(PLENS):
        row = tokens[b, : int(lens[b])].cpu()
        with torch.no_grad():
            full = ref(row.unsqueeze(0))[0]
        for t in range(p, int(lens[b])):
            lg = full[t - 1]
            assert lg[row[t]] >= lg.max() - margin * lg.abs().max(), (b, t)


def test_generate_ragged_gpu(cuda):
    from replicann_amd.models import gpt2 as G
    m = _model(cuda, 2)
    ref = _fp32(m)
    idx = _padded(cuda)
    # an untested first call: the GEMM autotuner settles each decode shape's kernel during it, so the
    # exact-equality comparisons below are between runs on the same kernels
    m.generate(idx, NEW, prompt_lens=PLENS, temperature=0, graph=False)
    runs = {}
    for graph in (True, False):
        tokens, lens = m.generate(idx, NEW, prompt_lens=PLENS, temperature=0, graph=graph)
        assert lens.tolist() == [p + NEW for p in PLENS] and tokens.shape == (3, max(PLENS) + NEW)
        for b, p in enumerate(PLENS):
            assert torch.equal(tokens[b, :p], idx[b, :p])
        _assert_greedy(ref, tokens, lens)
        assert len(m._decode_graphs()) <= G.DECODE_GRAPHS_MAX
        runs[graph] = (tokens.clone(), lens.clone())
    # whatever the padding holds changes nothing (rows are independent, the kernels deterministic)
    t2, l2 = m.generate(_padded(cuda, junk=True), NEW, prompt_lens=PLENS, temperature=0, graph=True)
    assert torch.equal(t2, runs[True][0]) and torch.equal(l2, runs[True][1])
    assert len(m._decode_graphs()) == 1  # the second ragged call replayed the stored step
    # EOS rerun: every row equals its no-EOS row up to and including its first EOS, pad after that
    for graph in (True, False):
        base = runs[graph][0]
        eos = int(base[0, PLENS[0] + 3])
        tokens, lens = m.generate(idx, NEW, prompt_lens=PLENS, eos_token_id=eos, temperature=0, graph=graph)
        assert tokens.shape[1] == int(lens.max())
        for b, p in enumerate(PLENS):
            gen = base[b, p: p + NEW].tolist()
            n = p + (gen.index(eos) + 1 if eos in gen else NEW)
            assert int(lens[b]) == n, (graph, b)
            assert torch.equal(tokens[b, :n], base[b, :n]), (graph, b)
            assert bool((tokens[b, n:] == eos).all())
        assert len(m._decode_graphs()) <= G.DECODE_GRAPHS_MAX
    # a uniform call afterwards: a plain tensor, its own registry entry
    out = m.generate(idx, NEW, temperature=0)
    assert torch.is_tensor(out) and out.shape == (3, max(PLENS) + NEW)
    assert len(m._decode_graphs()) <= G.DECODE_GRAPHS_MAX
    m.clear_decode_graphs()
