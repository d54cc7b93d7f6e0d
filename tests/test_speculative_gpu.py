"""Speculative decoding on the HIP kernels: the multi-query window attention kernel
(csrc/kernels/attention_window.hip) with its cache append, its binding, the window step of the model
(eager and captured) and ``GPT2.generate(draft=...)`` on the native (head size 64) and composed
(head size 32) paths.

Kernel shapes sit at the kernel's own edges: positions at the 16- and 32-key tile boundaries, the
empty cache, a cache that gives all four waves several tiles, and the last position at which a
16-row window fits a 1024-row buffer; window lengths 1, 2, an odd one and the full 16.

Tolerances: 1e-2 relative L2 for the attention (the bound tests/test_ops_gpu.py uses for the same
arithmetic), 3e-2 of the row's largest logit on the 2-layer bf16 model against its fp32 copy (stated
and derived in tests/test_generate_gpu.py).  No acceptance rate is asserted: bf16 near-ties between
the one-token GEMM and the window GEMM make it a measurement."""

import copy

import pytest
import torch

from replicann_amd import _ext, ops
from replicann_amd.models import decoding
from replicann_amd.models.decoding import KVCache

pytestmark = pytest.mark.gpu

PLENS = [5, 20, 13]
NEW = 12
B, H, L = 8, 2, 1024
POS = [0, 1, 15, 16, 31, 33, 255, 1008]
SCHEMA = "replicann_decode::attn_window(Tensor qkv, Tensor(a!) kv, Tensor pos, float scale) -> Tensor"


@pytest.fixture(autouse=True)
def _inference():
    """Everything here is inference: with grad on, ``ops.attention_window`` takes the composed path."""
    with torch.no_grad():
        yield


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _raw():
    _ext.ops()
    return torch.ops.replicann_decode.attn_window


# ------------------------------------------------------------------ the kernel
def _case(T, seed=0):
    """Host tensors: qkv (B, T, 3, H, 64) and a cache whose rows at and past pos[b] are NaN."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, 64, generator=g).bfloat16()
    kv = torch.randn(B, L, 2, H, 64, generator=g).bfloat16()
    for b, p in enumerate(POS):
        kv[b, p:] = float("nan")
    return qkv, kv


_REFS = {}


def _reference(T):
    """(qkv, kv, per-(row, query) fp32 reference (B, T, H, 64)), computed once per T and never changed."""
    if T not in _REFS:
        qkv, kv = _case(T)
        ref = torch.empty(B, T, H, 64)
        for b, p in enumerate(POS):
            for i in range(T):  # the query's own keys: cache rows < pos, window rows <= i
                k = torch.cat([kv[b, :p, 0], qkv[b, : i + 1, 1]]).unsqueeze(0).float()
                v = torch.cat([kv[b, :p, 1], qkv[b, : i + 1, 2]]).unsqueeze(0).float()
                ref[b, i] = ops.attention_reference(qkv[b: b + 1, i: i + 1, 0].float(), k, v, 0.125)[0, 0]
        _REFS[T] = (qkv, kv, ref)
    return _REFS[T]


def _on_gpu(cuda, qkv, kv):
    # qkv as a strided view (a batch stride that is not T rows), as out of a wider projection buffer
    wide = torch.zeros(B, qkv.shape[1] + 1, 3, H, 64, dtype=torch.bfloat16, device=cuda)
    wide[:, : qkv.shape[1]] = qkv.to(cuda)
    return wide[:, : qkv.shape[1]], kv.to(cuda)


@pytest.mark.parametrize("T", [1, 2, 5, 16])
def test_attention_window_kernel(cuda, T):
    qkv_h, kv_h, ref = _reference(T)
    qkv, kv = _on_gpu(cuda, qkv_h, kv_h)
    pos = torch.tensor(POS, device=cuda)
    out = _raw()(qkv, kv, pos, 0.125)  # the kernel itself
    assert out.shape == (B, T, H, 64) and out.dtype == torch.bfloat16
    assert bool(torch.isfinite(out).all())
    out_h = out.cpu()
    for b in range(B):
        for i in range(T):
            err = rel_err(out_h[b, i], ref[b, i])
            assert err < 1e-2, (b, i, err)
    # the buffer, bit for bit: the window rows are qkv's K|V, everything else (NaN rows included) is unchanged
    want = kv_h.clone()
    for b, p in enumerate(POS):
        want[b, p: p + T] = qkv_h[b, :, 1:3]
    assert torch.equal(kv.cpu().view(torch.int16), want.view(torch.int16))
    # two runs agree bit for bit (the second one from the same starting buffer)
    kv2 = kv_h.to(cuda)
    out2 = ops.attention_window(qkv, kv2, pos)  # the public op runs the same kernel
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(kv.view(torch.int16), kv2.view(torch.int16))
    # int32 positions: the same output
    out3 = ops.attention_window(qkv, kv_h.to(cuda), pos.int())
    assert torch.equal(out.view(torch.int16), out3.view(torch.int16))


def test_attention_window_one_token_matches_attention_decode(cuda):
    qkv_h, kv_h, _ = _reference(1)
    qkv, kv = _on_gpu(cuda, qkv_h, kv_h)
    pos = torch.tensor(POS, device=cuda)
    out = ops.attention_window(qkv, kv, pos)
    dec = ops.attention_decode(qkv[:, :, 0], kv[:, :, 0], kv[:, :, 1], lens=pos + 1)  # kv now holds the new row
    for b in range(B):
        assert rel_err(out[b], dec[b]) < 1e-2, b


def test_attention_window_clamps_positions(cuda):
    """Positions at the end of, past, before and far outside a 40-row buffer: only in-range rows are
    written and the memory on both sides of the buffer is untouched."""
    Lc, T, G = 40, 5, 4096
    pos_h = [38, 40, -1, 1 << 40]
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(4, T, 3, H, 64, generator=g).bfloat16().to(cuda)
    n = 4 * Lc * 2 * H * 64
    slab = torch.full((G + n + G,), 7.0, dtype=torch.bfloat16, device=cuda)  # guard | buffer | guard
    kv = slab[G: G + n].view(4, Lc, 2, H, 64)
    kv.copy_(torch.randn(4, Lc, 2, H, 64, generator=g).bfloat16())
    before = kv.cpu().clone()
    out = ops.attention_window(qkv, kv, torch.tensor(pos_h, device=cuda))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert bool((slab[:G] == 7.0).all()) and bool((slab[G + n:] == 7.0).all())
    want = before.clone()
    want[0, 38:40] = qkv[0, :2, 1:3].cpu()  # two rows fit
    want[2, 0:T] = qkv[2, :, 1:3].cpu()  # a negative position is row 0; rows 1 and 3 (pos >= L) write nothing
    assert torch.equal(kv.cpu().view(torch.int16), want.view(torch.int16))
    # the rows that did not fit are still attended (from qkv): row 0 is cache rows < 38 and the window so far
    for i in range(T):
        k = torch.cat([before[0, :38, 0], qkv[0, : i + 1, 1].cpu()]).unsqueeze(0).float()
        v = torch.cat([before[0, :38, 1], qkv[0, : i + 1, 2].cpu()]).unsqueeze(0).float()
        ref = ops.attention_reference(qkv[0:1, i: i + 1, 0].cpu().float(), k, v, 0.125)
        assert rel_err(out[0, i], ref[0, 0]) < 1e-2, i


def test_attn_window_binding_checks(cuda):
    op = _raw()
    qkv = torch.zeros(2, 3, 3, H, 64, dtype=torch.bfloat16, device=cuda)
    kv = torch.zeros(2, 64, 2, H, 64, dtype=torch.bfloat16, device=cuda)
    pos = torch.zeros(2, dtype=torch.long, device=cuda)
    assert op(qkv, kv, pos, 0.125).shape == (2, 3, H, 64)
    bad = [
        (torch.zeros(2, 17, 3, H, 64, dtype=torch.bfloat16, device=cuda), kv, pos),  # T
        (torch.zeros(2, 0, 3, H, 64, dtype=torch.bfloat16, device=cuda), kv, pos),
        (qkv[..., :32], kv[..., :32], pos),  # D
        (qkv.half(), kv.half(), pos),  # dtype
        (qkv, kv.float(), pos),
        (qkv, torch.zeros(2, 2048, 2, H, 64, dtype=torch.bfloat16, device=cuda), pos),  # L
        (qkv, kv[:, :, :1], pos),  # shapes
        (qkv, kv[:1], pos),
        (qkv, kv, pos[:1]),  # pos shape
        (qkv, kv, pos.view(2, 1)),
        (qkv, kv, pos.float()),  # pos dtype
        (qkv, kv, pos.cpu()),  # device
        (qkv[0], kv, pos),  # rank
        (qkv, kv[0], pos),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            op(*args, 0.125)


def test_attn_window_schema_and_dispatch_key_are_pinned():
    op = _raw()
    assert str(op.default._schema) == SCHEMA
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    assert has("replicann_decode::attn_window", "CUDA")
    assert not any(has("replicann_decode::attn_window", k) for k in ("CPU", "CompositeExplicitAutograd",
                                                                    "CompositeImplicitAutograd"))
    assert [n for n in torch._C._dispatch_get_all_op_names() if n.startswith("replicann_decode::")] == [
        "replicann_decode::attn_window"]


# ------------------------------------------------------------------ the model
def _model(cuda, n_head, seed=0):
    import replicann_amd as R
    torch.manual_seed(seed)
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


def _assert_greedy(ref, tokens, lens, margin=3e-2):
    for b, p in enumerate(PLENS):
        row = tokens[b, : int(lens[b])].cpu()
        with torch.no_grad():
            full = ref(row.unsqueeze(0))[0]
        for t in range(p, int(lens[b])):
            lg = full[t - 1]
            assert lg[row[t]] >= lg.max() - margin * lg.abs().max(), (b, t)


@pytest.mark.parametrize("n_head", [2, 4])
def test_decode_window_teacher_forced_gpu(cuda, n_head):
    """Windows (eager, then captured and replayed) with partial advances over stale rows: every greedy
    id is within the margin of the fp32 forward's best logit at the row's own position."""
    m = _model(cuda, n_head)
    ref = _fp32(m)
    g = torch.Generator().manual_seed(3)
    seq = torch.randint(0, 1000, (3, 48), generator=g)
    with torch.no_grad():
        full = ref(seq)  # (3, 48, vocab) fp32
    cache = KVCache(2, 64)
    idx = torch.stack([torch.cat([seq[b, :p], seq.new_zeros(max(PLENS) - p)]) for b, p in enumerate(PLENS)])
    m.decode_step(idx.to(cuda), cache, lens=PLENS)
    at = list(PLENS)

    def window(T, counts, run):
        toks = torch.stack([seq[b, at[b]: at[b] + T] for b in range(3)]).clone()
        for b, c in enumerate(counts):
            toks[b, c:] = 999  # not committed: must leave no trace
        ids = run(toks.to(cuda)).cpu()
        assert cache.pos_t.tolist() == at  # the window step does not move the position
        for b, c in enumerate(counts):
            for i in range(c):
                lg = full[b, at[b] + i]
                assert lg[ids[b, i]] >= lg.max() - 3e-2 * lg.abs().max(), (b, i)
        cache.advance(torch.tensor(counts, device=cuda))
        for b, c in enumerate(counts):
            at[b] += c
        assert cache.pos_t.tolist() == at and cache.lens.tolist() == [a + 1 for a in at]

    eager = lambda toks: m.decode_window(toks, cache)  # noqa: E731
    window(5, [5, 5, 5], eager)
    window(5, [1, 3, 0], eager)
    graph, tok, out = decoding.capture_window(m, cache, 3, 5)
    assert cache.pos_t.tolist() == at and cache.lens.tolist() == [a + 1 for a in at]  # positions as before the capture

    def replay(toks):
        tok.copy_(toks)
        graph.replay()
        return out.clone()

    window(5, [2, 5, 4], replay)
    window(5, [5, 0, 1], replay)
    logits = m.decode_step(torch.stack([seq[b, at[b]] for b in range(3)]).view(3, 1).to(cuda), cache)  # a one-token step
    for b in range(3):
        lg = full[b, at[b]]
        assert lg[int(logits[b].argmax())] >= lg.max() - 3e-2 * lg.abs().max(), b
    at = [a + 1 for a in at]
    window(5, [3, 3, 3], replay)


@pytest.mark.parametrize("n_head", [2, 4])
@pytest.mark.parametrize("which", ["same", "other"])
def test_generate_with_draft_gpu(cuda, n_head, which):
    m = _model(cuda, n_head)
    draft = m if which == "same" else _model(cuda, n_head, seed=7)
    ref = _fp32(m)
    idx = _padded(cuda)
    kw = dict(prompt_lens=PLENS, temperature=0, draft=draft, draft_k=4)
    # an untested first call: the GEMM autotuner settles each decode shape's kernel during it, so the
    # exact-equality comparisons below are between runs on the same kernels
    m.generate(idx, NEW, graph=False, **kw)
    runs = {}
    for graph in (True, False):
        stats = {}
        tokens, lens = m.generate(idx, NEW, graph=graph, stats=stats, **kw)
        assert lens.tolist() == [p + NEW for p in PLENS] and tokens.shape == (3, max(PLENS) + NEW)
        for b, p in enumerate(PLENS):
            assert torch.equal(tokens[b, :p], idx[b, :p])
            assert bool((tokens[b, p + NEW:] == 0).all())
        _assert_greedy(ref, tokens, lens)  # every committed token, whichever model proposed it
        assert 1 <= stats["rounds"] <= NEW - 1
        assert all(0 <= a <= d for a, d in zip(stats["accepted"].tolist(), stats["drafted"].tolist()))
        runs[graph] = tokens
    assert torch.equal(runs[True], runs[False])
    junk, _ = m.generate(_padded(cuda, junk=True), NEW, graph=True, **kw)
    assert torch.equal(junk, runs[True])  # whatever the padding holds
    # an EOS taken from the base run: each row equals it up to and including its first EOS, pad after
    eos = int(runs[True][1, PLENS[1] + 3])
    got, glens = m.generate(idx, NEW, graph=True, eos_token_id=eos, pad_token_id=0, **kw)
    for b, p in enumerate(PLENS):
        gen = runs[True][b, p: p + NEW].tolist()
        n = gen.index(eos) + 1 if eos in gen else NEW
        assert int(glens[b]) == p + n, b
        assert got[b, : p + n].tolist() == runs[True][b, : p + n].tolist(), b
        assert bool((got[b, p + n:] == 0).all()), b
    assert int(glens[1]) <= PLENS[1] + 4
    # uniform call: a plain tensor
    uni = m.generate(idx[:, :5], NEW, temperature=0, draft=draft, draft_k=2)
    assert torch.is_tensor(uni) and uni.shape == (3, 5 + NEW)
    for mm in {m, draft}:
        assert len(mm._decode_graphs()) <= decoding.DECODE_GRAPHS_MAX
    assert any("window" in k for k in m._decode_graphs())
