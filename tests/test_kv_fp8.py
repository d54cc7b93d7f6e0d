"""The fp8 KV cache on the CPU: the composed paths of ops.kv8 (the float reference of the kernels' semantics)
bitwise against tests/exact_fp8.py, and generation with ``kv_dtype="fp8"`` against a test-side loop that keeps a
float cache.  Cases and references: tests/kv8_cases.py."""

import copy

import pytest
import torch

import exact_fp8 as X
import kv8_cases as C
from exact_fp8 import E4M3

B, H, D, L = 3, 2, 64, 16


@pytest.fixture(scope="module")
def ops():
    from replicann_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------
# bytes and scales
# ------------------------------------------------------------------------------------------------
def test_inputs_hold_every_class():
    """What the byte cases feed: ties, subnormal results, saturating values at every k, and the two edge rows."""
    for k in X.KS:
        for cls in X.AMAX_CLASSES:
            A, scale, T, _ = C._table(k, cls)
            rep = X.table_report(T, E4M3, X.log2i(scale))
            assert rep["ties"] > 100 and rep["subnormal"] >= 14 and rep["underflow_tie"] == 2, (k, cls, rep)
    x, eb, es = C.head_rows(400, D)
    assert float(es[5]) == 1.0 and set(eb[5].tolist()) == {0x00, 0x80}
    assert float(es[9]) == 2.0**-126 and float(x[9].float().abs().max()) == 2.0**-120
    assert {float(s) for s in es} >= {2.0**k for k in (-20, -19, 0, 1, 10, 11)}
    # the planted maxima reach the top code, and subnormal results are plenty
    assert (eb & 0x7F).max() == 0x7E and int(((eb & 0x7F) < 8).sum()) > 1000


@pytest.mark.parametrize("T,pos", [(1, [0]), (5, [0]), (5, [0, 7, 13]), (4, [12, 15, 11]), (1, [3])])
def test_append_bytes(ops, T, pos):
    C.case_append(ops.kv8_append, "cpu", B, T, H, D, L, pos)


def test_append_int32_and_no_write_positions(ops):
    C.case_append(ops.kv8_append, "cpu", B, 3, H, D, L, [L, -1, 14], dtype=torch.int32)  # L, < 0: nothing; 14: 2 rows
    C.case_append(ops.kv8_append, "cpu", B, 2, H, D, L, [5000, -7, L])  # nothing at all


def test_emulation_agrees_and_wrong_ones_fail():
    """The check itself: torch's float8 casts (a second implementation) pass it; rounding toward zero or a scale
    rounded down must not."""
    C.case_append(C.emu_append(), "cpu", B, 5, H, D, L, [0, 7, 13])
    for slip in ("round_toward_zero", "scale_round_down"):
        with pytest.raises(AssertionError):
            C.case_append(C.emu_append(slip), "cpu", B, 5, H, D, L, [0, 7, 13])


def test_decode_bytes_and_sentinels(ops):
    """The attention op writes exactly the new row, with the bytes the append writes for the same vectors."""
    C.case_decode_bytes(ops.attention_decode_kv8, "cpu", B, H, D, L, steps=6, pos0=[0, 9, 12])  # row 2 runs past L
    C.case_decode_bytes(ops.attention_decode_kv8, "cpu", B, H, D, L, steps=2, pos0=[-3, L, 5000], dtype=torch.int32)
    kv8, sc = C.case_decode_bytes(ops.attention_decode_kv8, "cpu", B, H, D, L, steps=4, pos0=[2])  # one shared position
    x, _, _ = C.head_rows(4 * B * 2 * H, D)
    kv8b, scb = C.fresh_cache(B, L, H, D, "cpu")
    ops.kv8_append(x.view(4, B, 2, H, D).transpose(0, 1).contiguous(), kv8b, scb, torch.tensor([2]))
    assert torch.equal(kv8, kv8b) and torch.equal(sc, scb)


def test_decode_attention_value(ops):
    """Rows at or past pos hold the NaN byte under NaN scales; the output is the fp32 reference's."""
    pos = [0, 5, L]
    kv8, sc = C.random_cache(B, L, H, D, pos, "cpu")
    qkv = torch.randn(B, 1, 3, H, D, generator=torch.Generator().manual_seed(1))
    ref = C.attention_ref(qkv, kv8, sc, pos)
    for p in (torch.tensor(pos), torch.tensor(pos, dtype=torch.int32)):
        out = ops.attention_decode_kv8(qkv, kv8.clone(), sc.clone(), p)
        # both sides are fp32 over identical operands: 64-term dot products and a sum over <= 17 keys, in another order
        assert bool(torch.isfinite(out).all()) and C.rel_l2(out, ref) < 1e-5
    kv8, sc = C.random_cache(B, L, H, D, [5] * B, "cpu")
    one = ops.attention_decode_kv8(qkv, kv8.clone(), sc.clone(), torch.tensor([5]))
    same = ops.attention_decode_kv8(qkv, kv8.clone(), sc.clone(), torch.tensor([5] * B))
    assert bool(torch.isfinite(one).all()) and torch.equal(one, same)


def test_dequantize_exact(ops):
    """decode_table[byte] · scale for all 256 codes at every scale, bit for bit in bf16; NaN codes by class."""
    dec = X.decode_table(E4M3)
    for s in (2.0**-20, 1.0, 2.0**10):
        kv8 = torch.arange(256, dtype=torch.uint8).view(1, 2, 2, 1, 64)
        got = ops.kv8_dequantize(kv8, torch.full((1, 2, 2, 1), s))
        assert got.dtype == torch.bfloat16 and got.shape == kv8.shape
        exp = (dec * s).view(kv8.shape)
        nan = torch.isnan(exp)
        assert int(nan.sum()) == 2 and torch.equal(torch.isnan(got), nan)
        assert torch.equal(got.double()[~nan], exp[~nan])  # exact: the product is a bf16 value
        assert torch.equal(torch.signbit(got.float())[~nan], torch.signbit(exp)[~nan])


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
def _model():
    import replicann_amd as R
    torch.manual_seed(0)
    return R.GPT2(R.GPT2Config.tiny(n_embd=128, n_head=2, n_layer=2, block_size=128)).eval()


def _prompts():
    g = torch.Generator().manual_seed(3)
    lens = [5, 20, 13]
    idx = torch.randint(0, 1000, (3, 20), generator=g)
    return idx, lens


def _qdq(x):
    """Quantise / dequantise head rows with the references: ``encode`` at ``scale_ref``'s scale, ``decode_table``."""
    a = x.float().abs().amax(-1)
    scale = torch.tensor([X.scale_ref(v, E4M3) for v in a.reshape(-1).tolist()], dtype=torch.float64).view(a.shape)
    b8 = X.encode(x.double() / scale.unsqueeze(-1), E4M3)
    return (X.decode_table(E4M3)[b8.long()] * scale.unsqueeze(-1)).float()


def _ref_cache(n_layer, max_len):
    from replicann_amd import ops
    from replicann_amd.models.decoding import KVCache

    class RefCache(KVCache):
        """The positions of KVCache, and a float cache of quantised-then-dequantised rows in place of the bytes."""

        def __init__(self):
            super().__init__(n_layer, max_len, "fp8")
            self.rows = {}

        def step8(self, layer, qkv, causal):
            Bq, T, _, Hq, Dq = qkv.shape
            buf = self.rows.setdefault(layer, torch.zeros(Bq, self.max_len, 2, Hq, Dq))
            if self.kv[layer] is None:
                self.kv[layer] = buf  # (to_per_sequence asks kv[0] for the device)
            new = _qdq(qkv[:, :, 1:3])
            if T > 1:  # a prefill (or a later pass of several tokens) attends its own rows unquantised
                assert self.mode == "host"
                k, v = (torch.cat([buf[:, :self.pos, w], qkv[:, :, 1 + w]], 1) for w in (0, 1))
                buf[:, self.pos:self.pos + T] = new
                return ops.attention_reference(qkv[:, :, 0], k, v, Dq ** -0.5, causal=True)
            pos = [self.pos] * Bq if self.mode == "host" else self.pos_t.tolist()
            out = []
            for b, n in enumerate(pos):
                kv = torch.cat([buf[b, :n], new[b]], 0).unsqueeze(0)
                out.append(ops.attention_reference(qkv[b:b + 1, :, 0], kv[:, :, 0], kv[:, :, 1], Dq ** -0.5))
                if n < self.max_len:
                    buf[b, n] = new[b, 0]
            return torch.cat(out, 0)

    return RefCache()


def _ref_generate(model, idx, lens, new, eos=None):
    """Greedy generation, the loop written out: (each row's generated tokens, the logits of every step with the
    rows that were live at it)."""
    cache = _ref_cache(model.config.n_layer, model.config.block_size)
    Bq = idx.shape[0]
    with torch.no_grad():
        logits = model.decode_step(idx, cache, lens=lens) if lens is not None else model.decode_step(idx, cache)
        out, steps, done = [[] for _ in range(Bq)], [], [False] * Bq
        for i in range(new):
            steps.append((logits.clone(), [not d for d in done]))
            nxt = logits.argmax(-1)
            for b in range(Bq):
                if done[b]:
                    nxt[b] = eos  # a finished row emits the pad id (the EOS id)
                else:
                    out[b].append(int(nxt[b]))
                    done[b] = eos is not None and int(nxt[b]) == eos
            if i + 1 == new:
                break
            if cache.per_seq:
                cache.active.copy_(~torch.tensor(done))
            logits = model.decode_step(nxt.view(Bq, 1), cache)
    return out, steps


def _recorded(model, fn):
    """``fn()`` with the logits of every ``decode_step`` of ``model`` kept."""
    seen, orig = [], model.decode_step

    def rec(*a, **kw):
        lg = orig(*a, **kw)
        seen.append(lg.clone())
        return lg

    model.decode_step = rec
    try:
        return fn(), seen
    finally:
        del model.decode_step


def _compare(steps, seen):
    assert len(seen) >= 1 and len(seen) <= len(steps)
    for (ref, live), got in zip(steps, seen):
        live = torch.tensor(live)
        assert float((got[live] - ref[live]).abs().max()) <= 1e-5


def test_generate_uniform_matches_float_cache_loop():
    m = _model()
    idx, _ = _prompts()
    ref, steps = _ref_generate(m, idx, None, 12)
    out, seen = _recorded(m, lambda: m.generate(idx, 12, temperature=0, kv_dtype="fp8"))
    assert out[:, 20:].tolist() == ref
    _compare(steps, seen)


def test_generate_ragged_matches_float_cache_loop():
    m = _model()
    idx, lens = _prompts()
    ref, steps = _ref_generate(m, idx, lens, 12)
    (tokens, tl), seen = _recorded(m, lambda: m.generate(idx, 12, temperature=0, prompt_lens=lens, kv_dtype="fp8"))
    assert tl.tolist() == [n + 12 for n in lens]
    for b, n in enumerate(lens):
        assert tokens[b, n:n + 12].tolist() == ref[b]
    _compare(steps, seen)
    rows = m.generate_batch([idx[b, :n] for b, n in enumerate(lens)], 12, temperature=0, kv_dtype="fp8")
    assert [r[n:].tolist() for r, n in zip(rows, lens)] == ref


def test_generate_ragged_eos_matches_float_cache_loop():
    m = _model()
    idx, lens = _prompts()
    free, _ = _ref_generate(m, idx, lens, 12)
    eos = free[0][0]  # row 0 stops at once and rewrites its own cache row from then on; the others run on
    ref, steps = _ref_generate(m, idx, lens, 12, eos=eos)
    assert len(ref[0]) == 1 and max(map(len, ref)) == 12
    (tokens, tl), seen = _recorded(m, lambda: m.generate(idx, 12, temperature=0, prompt_lens=lens, eos_token_id=eos,
                                                         kv_dtype="fp8"))
    assert tl.tolist() == [n + len(r) for n, r in zip(lens, ref)]
    for b, n in enumerate(lens):
        assert tokens[b, n:n + len(ref[b])].tolist() == ref[b]
    _compare(steps, seen)


def test_draft_with_fp8_raises_and_bad_dtype():
    m = _model()
    idx, _ = _prompts()
    with pytest.raises(ValueError, match="fp8"):
        m.generate(idx, 4, temperature=0, draft=_model(), kv_dtype="fp8")
    with pytest.raises(ValueError, match="kv_dtype"):
        m.generate(idx, 4, temperature=0, kv_dtype="int8")
    from replicann_amd.models.decoding import KVCache
    with pytest.raises(ValueError, match="kv_dtype"):
        KVCache(2, 16, kv_dtype="e5m2")


def test_bf16_generation_unchanged_after_fp8():
    m = _model()
    fresh = copy.deepcopy(m)
    idx, lens = _prompts()
    m.generate(idx, 12, temperature=0, kv_dtype="fp8")
    m.generate(idx, 12, temperature=0, prompt_lens=lens, kv_dtype="fp8")
    a, sa = _recorded(m, lambda: m.generate(idx, 12, temperature=0))
    b, sb = _recorded(fresh, lambda: fresh.generate(idx, 12, temperature=0))
    assert torch.equal(a, b) and len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))


def test_slow_path_matches_float_cache():
    """T > 1 at pos > 0 (host mode): the cached rows dequantised, this pass's own rows unquantised, then the append."""
    from replicann_amd.models.decoding import KVCache
    m = _model()
    idx, _ = _prompts()
    tail = torch.randint(0, 1000, (3, 3), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        a, r = KVCache(2, 32, "fp8"), _ref_cache(2, 32)
        for cache in (a, r):
            m.decode_step(idx[:, :9], cache)
        got, ref = m.decode_step(tail, a), m.decode_step(tail, r)
        assert a.pos == r.pos == 12 and float((got - ref).abs().max()) <= 1e-5
        got, ref = m.decode_step(tail[:, :1], a), m.decode_step(tail[:, :1], r)  # and it left the rows a step reads
        assert float((got - ref).abs().max()) <= 1e-5
    for layer in range(2):
        deq = C.dequantize_ref(a.kv[layer][:, :13], a.kv_scale[layer][:, :13]).float()
        assert torch.equal(deq, r.rows[layer][:, :13])
