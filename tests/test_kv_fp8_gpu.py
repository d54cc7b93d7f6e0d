"""The fp8 KV cache on the GPU: the kernels of csrc/kernels/attention_decode_kv8.hip byte for byte against
tests/exact_fp8.py, the attention at the kernel's own edges against an fp32 reference over the dequantised rows,
the composed path at a head size the kernel does not take, and generation with ``kv_dtype="fp8"``.  Cases and
references: tests/kv8_cases.py.  Every op call goes through the ``ops`` fixture, which asserts that a call the kernels
take reached ``torch.ops.replicann_kv8`` (and that a composed one did not): the byte cases are about the kernels.

Bounds: the attention output within 1e-2 relative L2 of ``ops.attention_reference`` in fp32 over identical operands
(the bound of this arithmetic throughout the project: bf16 output rounding, fp32 summation order); the 2-layer bf16
model's logits within 3e-2 relative L2 of the fp32 CPU model run with the same fp8 cache (the bound stated and
derived in tests/test_generate_gpu.py)."""

import copy

import pytest
import torch

import kv8_cases as C

pytestmark = pytest.mark.gpu

B, H, D, L = 4, 2, 64, 64
EDGE_N = (1, 31, 33, 64, 255, 257, 1000, 1024)  # keys read, the new row included: tests/test_decode_ragged_gpu.py's


class _Ops:
    """``replicann_amd.ops`` with every call checked for the path it took: a call that the kernels take (bf16, head
    size 64, L <= 1024) must reach ``torch.ops.replicann_kv8`` exactly once, any other must not.  The byte and edge
    cases below are about the kernels, not about the composed path."""

    def __init__(self, monkeypatch):
        from replicann_amd import ops
        from replicann_amd.ops import kv8
        self.ops, self.calls = ops, {"append": 0, "attn_decode": 0}
        raw, calls = kv8._raw(), self.calls

        class Counted:
            def __getattr__(self, name):
                def call(*a):
                    calls[name] += 1
                    return getattr(raw, name)(*a)
                return call

        monkeypatch.setattr(kv8, "_raw", lambda: Counted())

    def _expect(self, name, takes, fn, *a):
        before = self.calls[name]
        out = fn(*a)
        assert self.calls[name] - before == int(takes), f"{name}: the kernel was {'not ' if takes else ''}run"
        return out

    def kv8_append(self, kv_new, kv8, sc, pos):
        return self._expect("append", kv_new.shape[-1] == 64, self.ops.kv8_append, kv_new, kv8, sc, pos)

    def attention_decode_kv8(self, qkv, kv8, sc, pos):
        takes = qkv.shape[-1] == 64 and kv8.shape[1] <= 1024
        return self._expect("attn_decode", takes, self.ops.attention_decode_kv8, qkv, kv8, sc, pos)


@pytest.fixture
def ops(monkeypatch):
    return _Ops(monkeypatch)


def test_inference_only(cuda):
    """No silent fall-back: with grad enabled the kernels still run, and an input that requires grad is an error."""
    from replicann_amd import ops as O
    qkv = torch.zeros(2, 1, 3, H, D, dtype=torch.bfloat16, device=cuda)
    kv8, sc = C.fresh_cache(2, L, H, D, cuda)
    pos = torch.zeros(2, dtype=torch.long, device=cuda)
    assert torch.is_grad_enabled()
    with pytest.raises(RuntimeError, match="inference only"):
        O.attention_decode_kv8(qkv.clone().requires_grad_(), kv8, sc, pos)
    with pytest.raises(RuntimeError, match="inference only"):
        O.kv8_append(qkv[:, :, 1:3].clone().requires_grad_(), kv8, sc, pos)


# ------------------------------------------------------------------------------------------------
# 1. bytes, scales and sentinels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 5, 20])
@pytest.mark.parametrize("pos", [[0], [0, 7, 44, 63]])
def test_append_bytes(ops, cuda, T, pos):
    C.case_append(ops.kv8_append, cuda, B, T, H, D, L, pos, start=100 * T)  # at 63 only one row still fits


def test_append_int32_and_no_write_positions(ops, cuda):
    C.case_append(ops.kv8_append, cuda, B, 3, H, D, L, [L, -1, 62, 5000], dtype=torch.int32)
    C.case_append(ops.kv8_append, cuda, B, 2, H, D, L, [-5])


def test_append_strided_input(ops, cuda):
    """The K | V slice of a packed projection output, as the prefill passes it."""
    x, eb, es = C.head_rows(B * 5 * 2 * H, D, start=7)
    qkv = torch.zeros(B, 5, 3, H, D, dtype=torch.bfloat16, device=cuda)
    qkv[:, :, 1:3] = x.view(B, 5, 2, H, D).to(cuda)
    kv8, sc = C.fresh_cache(B, L, H, D, cuda)
    exp8, exp_sc = kv8.cpu().clone(), sc.cpu().clone()
    C.expect_written(exp8, exp_sc, eb.view(B, 5, 2, H, D), es.view(B, 5, 2, H), [3, 0, 60, 17], L)
    ops.kv8_append(qkv[:, :, 1:3], kv8, sc, torch.tensor([3, 0, 60, 17], device=cuda))
    C.assert_cache("strided append", kv8, sc, exp8, exp_sc)


def test_decode_bytes_and_sentinels(ops, cuda):
    """Every call writes exactly its own row — with the bytes the append writes for the same vectors."""
    C.case_decode_bytes(ops.attention_decode_kv8, cuda, B, H, D, L, steps=12, pos0=[0, 7, 44, 60])  # row 3 runs past L
    C.case_decode_bytes(ops.attention_decode_kv8, cuda, B, H, D, L, steps=2, pos0=[-3, L, 5000, L - 1],
                        dtype=torch.int32)
    kv8, sc = C.case_decode_bytes(ops.attention_decode_kv8, cuda, B, H, D, L, steps=6, pos0=[9])
    x, _, _ = C.head_rows(6 * B * 2 * H, D)
    kv8b, scb = C.fresh_cache(B, L, H, D, cuda)
    ops.kv8_append(x.view(6, B, 2, H, D).transpose(0, 1).contiguous().to(cuda), kv8b, scb,
                   torch.tensor([9], device=cuda))
    assert torch.equal(kv8, kv8b) and torch.equal(sc.view(torch.int32), scb.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# 2. the attention at the kernel's edges
# ------------------------------------------------------------------------------------------------
EB, EL = 8, 1024


def _edge_case(ops, cuda, pos, dtype, seed=1):
    """One call at ``pos`` (EB host integers) on a cache whose rows at or past pos hold 0x7F under NaN scales:
    finite, within 1e-2 of the reference, the written row right and nothing else touched.  Returns (qkv, the cache
    before, the output, the cache after)."""
    kv8, sc = C.random_cache(EB, EL, H, D, pos, cuda)
    qkv = torch.randn(EB, 1, 3, H, D, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).to(cuda)
    before = (kv8.clone(), sc.clone())
    out = ops.attention_decode_kv8(qkv, kv8, sc, torch.tensor(pos, dtype=dtype, device=cuda))
    assert out.shape == (EB, 1, H, D) and out.dtype == torch.bfloat16
    assert bool(torch.isfinite(out).all())
    ref = C.attention_ref(qkv, before[0], before[1], pos)
    err = C.rel_l2(out, ref)
    print(f"kv8 attention pos={sorted(set(pos))}: rel L2 {err:.3e}")
    assert err < 1e-2, err
    exp8, exp_sc = before[0].cpu().clone(), before[1].cpu().clone()
    nb, ns = C.quantize_ref(qkv[:, :, 1:3].float().cpu())
    C.expect_written(exp8, exp_sc, nb, ns, pos, EL)
    C.assert_cache(f"edge pos={pos}", kv8, sc, exp8, exp_sc)
    return qkv, before, out, (kv8, sc)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("n", EDGE_N)
def test_attention_edges(ops, cuda, n, dtype):
    pos = [n - 1] * EB
    qkv, before, out, after = _edge_case(ops, cuda, pos, dtype)
    # a second call with the same inputs: the same output and the same cache (the row in registers is the row in memory)
    again = ops.attention_decode_kv8(qkv, after[0], after[1], torch.tensor(pos, dtype=dtype, device=cuda))
    assert torch.equal(again, out)
    kv8, sc = (t.clone() for t in before)
    one = ops.attention_decode_kv8(qkv, kv8, sc, torch.tensor([n - 1], dtype=dtype, device=cuda))  # one shared position
    assert torch.equal(one, out)
    assert torch.equal(kv8, after[0]) and torch.equal(sc.view(torch.int32), after[1].view(torch.int32))


def test_attention_every_edge_in_one_batch(ops, cuda):
    _edge_case(ops, cuda, [n - 1 for n in EDGE_N], torch.int64, seed=2)


def test_attention_position_clamps(ops, cuda):
    """pos = 5000 is pos = L: every row read, nothing written."""
    qkv, before, out, after = _edge_case(ops, cuda, [EL] * EB, torch.int64, seed=3)
    assert torch.equal(after[0], before[0])
    kv8, sc = (t.clone() for t in before)
    big = ops.attention_decode_kv8(qkv, kv8, sc, torch.tensor([5000] * EB, device=cuda))
    assert torch.equal(big, out) and torch.equal(kv8, before[0])


def test_raw_op_rejects_bad_arguments(ops, cuda):
    op = torch.ops.replicann_kv8.attn_decode
    qkv = torch.zeros(2, 1, 3, H, D, dtype=torch.bfloat16, device=cuda)
    kv8, sc = C.fresh_cache(2, L, H, D, cuda)
    pos = torch.zeros(2, dtype=torch.long, device=cuda)
    op(qkv, kv8, sc, pos, 0.125)
    bad = [
        (qkv.float(), kv8, sc, pos),  # dtype
        (qkv, kv8.to(torch.int8), sc, pos),
        (qkv, kv8, sc.double(), pos),
        (qkv, kv8, sc, pos.float()),
        (qkv, kv8, sc, torch.zeros(3, dtype=torch.long, device=cuda)),  # neither 1 nor B positions
        (qkv, kv8.transpose(1, 2), sc, pos),  # layout
        (qkv, kv8[:, :, :, :, 1:], sc, pos),  # shape, alignment
        (qkv, kv8, sc[:, :, :, :1], pos),
        (qkv, kv8, sc, pos.cpu()),  # device
        (qkv[0], kv8, sc, pos),  # rank
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            op(*args, 0.125)


# ------------------------------------------------------------------------------------------------
# 3. a head size the kernel does not take: the composed path on the GPU
# ------------------------------------------------------------------------------------------------
def test_head_size_32_composed(ops, cuda):
    C.case_append(ops.kv8_append, cuda, B, 5, H, 32, L, [0, 7, 44, 63])
    C.case_append(ops.kv8_append, cuda, B, 2, H, 32, L, [L, -1, 62, 5000], dtype=torch.int32)
    C.case_decode_bytes(ops.attention_decode_kv8, cuda, B, H, 32, L, steps=4, pos0=[0, 7, 44, 62])
    pos = [0, 30, 63, L]
    kv8, sc = C.random_cache(B, L, H, 32, pos, cuda, seed=4)
    qkv = torch.randn(B, 1, 3, H, 32, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).to(cuda)
    ref = C.attention_ref(qkv, kv8, sc, pos)
    out = ops.attention_decode_kv8(qkv, kv8, sc, torch.tensor(pos, device=cuda))
    assert bool(torch.isfinite(out).all())
    err = C.rel_l2(out, ref)
    print(f"kv8 attention D=32 composed: rel L2 {err:.3e}")
    assert err < 1e-2, err


# ------------------------------------------------------------------------------------------------
# 4. the model
# ------------------------------------------------------------------------------------------------
def _model(cuda):
    import replicann_amd as R
    torch.manual_seed(0)
    m = R.GPT2(R.GPT2Config.tiny(n_embd=128, n_head=2, n_layer=2, block_size=128)).to(cuda)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m.eval()


def _cpu_twin(m):
    return copy.deepcopy(m).float().cpu().eval()


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _committed(cache, layer, n):
    return cache.kv[layer][:, :n], cache.kv_scale[layer][:, :n].view(torch.int32)


def test_steps_match_fp32_cpu_model(ops, cuda):
    """Teacher-forced: prefill 20, then 12 one-token steps, eager (host position) and captured (device position),
    every step's logits against the fp32 CPU model run with the same kind of cache; the two GPU caches agree
    bitwise on the committed rows."""
    from replicann_amd.models.decoding import KVCache
    m = _model(cuda)
    ref = _cpu_twin(m)
    seq = torch.randint(0, 1000, (3, 32), generator=torch.Generator().manual_seed(1))
    host, dev, cpu = (KVCache(2, 32, "fp8") for _ in range(3))
    want = ref.decode_step(seq[:, :20], cpu)
    seq_d = seq.to(cuda)
    assert rel_err(m.decode_step(seq_d[:, :20], host), want) < 3e-2
    m.decode_step(seq_d[:, :20], dev)
    g, tok, out = m._capture_decode(dev, 3)
    assert dev.mask is None  # no key mask, no index_fill_ in the graph: the kernel reads pos + 1 rows
    for t in range(20, 32):
        want = ref.decode_step(seq[:, t:t + 1], cpu)
        a = m.decode_step(seq_d[:, t:t + 1], host)
        tok.copy_(seq_d[:, t:t + 1])
        g.replay()
        ea, eg = rel_err(a, want), rel_err(out, want)
        print(f"kv8 step {t}: eager {ea:.3e} captured {eg:.3e}")
        assert ea < 3e-2 and eg < 3e-2, t
    torch.cuda.synchronize()
    assert int(dev.pos_t) == 32 and host.pos == 32
    # the GPU model ran the kernels: 2 layers x (2 prefills; 12 eager steps + the capture's warm-up and recording)
    assert ops.calls == {"append": 4, "attn_decode": 2 * (12 + 2)}
    for layer in range(2):
        for x, y in zip(_committed(host, layer, 32), _committed(dev, layer, 32)):
            assert torch.equal(x, y), layer


def test_generate_graph_matches_eager(cuda):
    m = _model(cuda)
    idx = torch.randint(0, 1000, (3, 20), device=cuda)
    e = m.generate(idx, 12, temperature=0, graph=False, kv_dtype="fp8")
    r = m.generate(idx, 12, temperature=0, graph=True, kv_dtype="fp8")
    assert e.shape == (3, 32) and torch.equal(e, r)
    assert torch.equal(m.generate(idx, 12, temperature=0, graph=True, kv_dtype="fp8"), r)  # the stored graph


def test_prefill_and_steps_leave_the_same_layer0_bytes(cuda):
    """Layer 0's keys / values depend on the embeddings alone, so a prefill of T tokens (kv8_append) and T one-token
    steps (the attention kernel's append) must leave the same bytes there.  Deeper layers legitimately differ: the
    prefill attends this pass's unquantised K / V, the steps attend the quantised rows."""
    from replicann_amd.models.decoding import KVCache
    m = _model(cuda)
    seq = torch.randint(0, 1000, (3, 20), device=cuda)
    a, b = KVCache(2, 32, "fp8"), KVCache(2, 32, "fp8")
    m.decode_step(seq, a)
    for t in range(20):
        m.decode_step(seq[:, t:t + 1], b)
    for x, y in zip(_committed(a, 0, 20), _committed(b, 0, 20)):
        assert torch.equal(x, y)


def test_generate_ragged_eos(cuda):
    m = _model(cuda)
    g = torch.Generator().manual_seed(3)
    lens = [5, 20, 13]
    idx = torch.randint(0, 1000, (3, 20), generator=g).to(cuda)
    free, fl = m.generate(idx, 12, temperature=0, prompt_lens=lens, kv_dtype="fp8", graph=False)
    assert fl.tolist() == [n + 12 for n in lens]
    eos = int(free[0, lens[0]])  # row 0 stops at once and rewrites its own cache row from then on
    e, el = m.generate(idx, 12, temperature=0, prompt_lens=lens, eos_token_id=eos, kv_dtype="fp8", graph=False)
    r, rl = m.generate(idx, 12, temperature=0, prompt_lens=lens, eos_token_id=eos, kv_dtype="fp8", graph=True)
    assert el.tolist()[0] == lens[0] + 1 and torch.equal(el, rl) and torch.equal(e, r)
    for b, n in enumerate(lens):  # the rows that run on are the free run's
        k = int(el[b]) - n
        assert torch.equal(e[b, n:n + k], free[b, n:n + k])


def test_native_sampler_captured_with_the_fp8_step(cuda):
    from replicann_amd.ops import rng
    m = _model(cuda)
    idx = torch.randint(0, 1000, (3, 20), device=cuda)
    kw = dict(temperature=0.9, top_k=50, sampler="native", kv_dtype="fp8", graph=True)
    rng.manual_seed(5)
    a = m.generate(idx, 12, **kw)  # captures
    rng.manual_seed(5)
    b = m.generate(idx, 12, **kw)  # replays
    rng.manual_seed(6)
    c = m.generate(idx, 12, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert len(m._decode_graphs()) == 1 and next(iter(m._decode_graphs()))[-2:] == ("sampler", "fp8")


def test_slow_path_matches_cpu(cuda):
    """A 3-token decode_step at position 9: the composed path over the dequantised rows."""
    from replicann_amd.models.decoding import KVCache
    m = _model(cuda)
    ref = _cpu_twin(m)
    seq = torch.randint(0, 1000, (3, 12), generator=torch.Generator().manual_seed(2))
    a, c = KVCache(2, 32, "fp8"), KVCache(2, 32, "fp8")
    m.decode_step(seq[:, :9].to(cuda), a)
    ref.decode_step(seq[:, :9], c)
    err = rel_err(m.decode_step(seq[:, 9:].to(cuda), a), ref.decode_step(seq[:, 9:], c))
    print(f"kv8 slow path: {err:.3e}")
    assert a.pos == 12 and err < 3e-2


def test_registry_keeps_fp8_and_bf16_apart(cuda):
    m = _model(cuda)
    fresh = copy.deepcopy(m)
    idx = torch.randint(0, 1000, (3, 20), device=cuda)
    m.generate(idx, 12, temperature=0, kv_dtype="fp8")
    a = m.generate(idx, 12, temperature=0)
    keys = list(m._decode_graphs())
    assert len(keys) == 2 and sum(k[-1] == "fp8" for k in keys) == 1 and keys[0][:5] == keys[1][:5]
    assert torch.equal(a, fresh.generate(idx, 12, temperature=0))
    caches = [e[0] for e in m._decode_graphs().values()]
    assert {c.kv[0].dtype for c in caches} == {torch.uint8, torch.bfloat16}
    with pytest.raises(ValueError, match="fp8"):
        m.generate(idx, 4, temperature=0, draft=fresh, kv_dtype="fp8")


# ------------------------------------------------------------------------------------------------
# 5. the bindings
# ------------------------------------------------------------------------------------------------
def test_schema_and_dispatch_keys(cuda):
    from replicann_amd import _ext
    _ext.ops()
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("replicann_kv8::"))
    assert names == ["replicann_kv8::append", "replicann_kv8::attn_decode"]
    assert str(torch.ops.replicann_kv8.attn_decode.default._schema) == (
        "replicann_kv8::attn_decode(Tensor qkv, Tensor(a!) kv8, Tensor(b!) kv_scale, Tensor pos, float scale) -> Tensor")
    assert str(torch.ops.replicann_kv8.append.default._schema) == (
        "replicann_kv8::append(Tensor kv_new, Tensor(a!) kv8, Tensor(b!) kv_scale, Tensor pos) -> ()")
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for n in names:
        assert has(n, "CUDA")
        assert not any(has(n, k) for k in ("CPU", "CompositeExplicitAutograd", "CompositeImplicitAutograd"))
    assert [n for n in torch._C._dispatch_get_all_op_names() if n.startswith("replicann_decode::")] == [
        "replicann_decode::attn_window"]
    assert [n for n in torch._C._dispatch_get_all_op_names() if n.startswith("replicann_spec::")] == [
        "replicann_spec::verify"]
