"""n samples per prompt over one shared prompt KV cache on the GPU: the two kernels of
csrc/kernels/attention_decode_prefix.hip at their own edges against the fp32 row-by-row reference
(tests/prefix_cases.py), the exact and bitwise properties, the raw op's argument checks, the composed path at a head
size the kernels do not take, and ``generate(num_samples=n)``.  Every op call goes through the ``ops`` fixture, which
asserts that a call the kernels take reached ``torch.ops.replicann_prefix`` exactly once (and that a composed one did
not).

Bounds: the attention output within 1e-2 relative L2 of ``ops.attention_reference`` in fp32 over identical operands
(the bound of this arithmetic throughout the project, stated in tests/test_kv_fp8_gpu.py: bf16 probabilities and
output rounding, fp32 summation order); the 2-layer bf16 model's logits within 3e-2 relative L2 of the fp32 CPU model
run with a plain cache on the repeated prompts (the bound stated and derived in tests/test_generate_gpu.py)."""

import copy

import pytest
import torch

import prefix_cases as C

pytestmark = pytest.mark.gpu

H, D, P, L = 2, 64, 1024, 256
BF = torch.bfloat16


class _Ops:
    """``ops.attention_decode_prefix`` with every call checked for the path it took."""

    def __init__(self, monkeypatch):
        from replicann_amd import ops
        from replicann_amd.ops import prefix
        self.ops, self.calls = ops, {"attn_decode": 0}
        raw, calls = prefix._raw(), self.calls

        class Counted:
            def __getattr__(self, name):
                def call(*a):
                    calls[name] += 1
                    return getattr(raw, name)(*a)
                return call

        monkeypatch.setattr(prefix, "_raw", lambda: Counted())

    def attention_decode_prefix(self, qkv, prefix_kv, plen, kv, pos, takes=None):
        if takes is None:
            takes = qkv.shape[-1] == 64 and qkv.shape[0] // prefix_kv.shape[0] <= 64
        before = self.calls["attn_decode"]
        out = self.ops.attention_decode_prefix(qkv, prefix_kv, plen, kv, pos)
        assert self.calls["attn_decode"] - before == int(takes), f"the kernels were {'not ' if takes else ''}run"
        return out


@pytest.fixture
def ops(monkeypatch):
    return _Ops(monkeypatch)


def _t(v, cuda, dtype=torch.int64):
    return torch.tensor(v, dtype=dtype, device=cuda)


# ------------------------------------------------------------------------------------------------
# 1. the attention at the kernels' edges
# ------------------------------------------------------------------------------------------------
# (G, n, prefix_len per group, pos per row or one value for all).  prefix_len: the tile (32), the split chunk and
# P; pos: the wave (64), the block (256 = L); n: one column, a padded block, a full one, a second block with one
# column, three blocks, four full ones
EDGES = {
    "empty-prefix-empty-tail": (1, 1, [0], 0),
    "one-prefix-row": (1, 2, [1], 1),
    "tile-minus-1": (1, 15, [31], 31),
    "tile": (1, 16, [32], 33),
    "tile-plus-1": (1, 17, [33], 255),
    "two-splits-minus-1": (1, 33, [255], L),
    "two-splits-plus-1": (1, 64, [257], 0),
    "last-split-partly": (3, 2, [1000, 1000, 1000], 31),
    "full": (1, 64, [P], L),
    "full-3-groups": (3, 17, [P, P, P], 33),
    "ragged-groups-and-rows": (3, 5, [0, 257, 1000], [0, 1, 31, 33, 255, L, 7, 0, 100, 64, 65, 63, 2, L, 128]),
    "ragged-33": (3, 33, [33, 1, 1024], [(7 * b) % (L + 1) for b in range(99)]),
}


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("name", list(EDGES))
def test_attention_edges(ops, cuda, name, index_dtype):
    G, n, plen, pos = EDGES[name]
    pos = pos if isinstance(pos, list) else [pos] * (G * n)
    out, ref, (qkv, before) = C.run_case(ops.attention_decode_prefix, G, n, H, D, P, L, plen, pos, BF, cuda, index_dtype,
                                         seed=len(name))
    err = C.rel_l2(out, ref)
    print(f"prefix attention {name}: rel L2 {err:.3e}")
    assert err < 1e-2, err
    # two runs agree bitwise
    prefix, kv = (t.clone() for t in before)
    again = ops.attention_decode_prefix(qkv, prefix, _t(plen, cuda, index_dtype), kv, _t(pos, cuda, index_dtype))
    assert torch.equal(C.bits(again), C.bits(out))


def test_single_key_is_the_value_row(ops, cuda):
    """prefix_len = 0 and pos = 0: the softmax over the one key is 1 and the output the new V row, bit for bit."""
    for G, n in ((1, 1), (3, 17), (1, 64)):
        qkv, prefix, kv = C.make(G, n, H, D, P, L, [0] * G, [0] * (G * n), BF, cuda, seed=n)
        out = ops.attention_decode_prefix(qkv, prefix, _t([0] * G, cuda), kv, _t([0] * (G * n), cuda))
        assert torch.equal(C.bits(out), C.bits(qkv[:, :, 2]))


def test_lengths_clamp(ops, cuda):
    """prefix_len = 5000 gives the bits of prefix_len = P; pos = L + 7 the bits of pos = L, and writes nothing."""
    G, n = 2, 3
    qkv, prefix, kv = C.make(G, n, H, D, P, L, [P] * G, [L] * (G * n), BF, cuda, seed=4)
    before = kv.clone()
    want = ops.attention_decode_prefix(qkv, prefix, _t([P] * G, cuda), kv, _t([L] * 6, cuda))
    assert torch.equal(C.bits(kv), C.bits(before))
    big = ops.attention_decode_prefix(qkv, prefix, _t([5000] * G, cuda), kv, _t([L + 7] * 6, cuda))
    assert torch.equal(C.bits(big), C.bits(want)) and torch.equal(C.bits(kv), C.bits(before))
    err = C.rel_l2(want, C.reference(qkv, prefix, before, [P] * G, [L] * 6))
    assert err < 1e-2, err


# ------------------------------------------------------------------------------------------------
# 2. sample independence
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 64])
def test_identical_samples_give_identical_rows(ops, cuda, n):
    """Padded columns and the second and later query blocks compute what the first column does."""
    plen, pos = 300, 37
    qkv, prefix, kv = C.make(1, n, H, D, P, L, [plen], [pos] * n, BF, cuda, seed=n)
    qkv, kv = qkv[:1].repeat(n, 1, 1, 1, 1), kv[:1].repeat(n, 1, 1, 1, 1)
    out = ops.attention_decode_prefix(qkv, prefix, _t([plen], cuda), kv, _t([pos] * n, cuda))
    assert bool(torch.isfinite(out).all())
    assert bool((C.bits(out) == C.bits(out[:1])).all())


def test_a_row_changes_no_other_row(ops, cuda):
    n, plen = 17, 300
    pos = [(5 * b) % 60 for b in range(n)]
    qkv, prefix, kv = C.make(1, n, H, D, P, L, [plen], pos, BF, cuda, seed=1)
    a = ops.attention_decode_prefix(qkv, prefix, _t([plen], cuda), kv.clone(), _t(pos, cuda))
    q2, k2 = qkv.clone(), kv.clone()
    q2[9], k2[9, :pos[9]] = -q2[9], -k2[9, :pos[9]]
    b = ops.attention_decode_prefix(q2, prefix, _t([plen], cuda), k2, _t(pos, cuda))
    others = [i for i in range(n) if i != 9]
    assert torch.equal(C.bits(a[others]), C.bits(b[others])) and not torch.equal(C.bits(a[9]), C.bits(b[9]))


def test_permuting_the_groups_permutes_the_output(ops, cuda):
    G, n, plen = 3, 5, [40, 1000, 257]
    pos = [(11 * b) % 70 for b in range(G * n)]
    qkv, prefix, kv = C.make(G, n, H, D, P, L, plen, pos, BF, cuda, seed=2)
    a = ops.attention_decode_prefix(qkv, prefix, _t(plen, cuda), kv.clone(), _t(pos, cuda))
    perm = [2, 0, 1]
    rows = [g * n + s for g in perm for s in range(n)]
    b = ops.attention_decode_prefix(qkv[rows], prefix[perm], _t([plen[g] for g in perm], cuda), kv[rows].clone(),
                                    _t([pos[r] for r in rows], cuda))
    assert torch.equal(C.bits(b), C.bits(a[rows]))


# ------------------------------------------------------------------------------------------------
# 3. the bindings
# ------------------------------------------------------------------------------------------------
def test_raw_op_rejects_bad_arguments(cuda):
    from replicann_amd import _ext
    _ext.ops()
    op = torch.ops.replicann_prefix.attn_decode
    qkv, prefix, kv = C.make(2, 2, H, D, 64, 32, [3, 3], [1] * 4, BF, cuda)
    plen, pos = _t([3, 3], cuda), _t([1] * 4, cuda)
    op(qkv, prefix, plen, kv, pos, 0.125)
    wide = torch.zeros(4, 32, 2, H, 72, dtype=BF, device=cuda)
    bad = [
        (qkv.float(), prefix, plen, kv, pos),  # dtypes
        (qkv, prefix.float(), plen, kv, pos),
        (qkv, prefix, plen, kv.to(torch.float16), pos),
        (qkv, prefix, plen.float(), kv, pos),
        (qkv, prefix, plen, kv, pos.to(torch.int16)),
        (qkv[:3], prefix, plen, kv[:3], pos[:3]),  # B not a multiple of G
        (qkv, prefix[:, :, :, :1], plen, kv, pos),  # H
        (qkv, prefix, plen, torch.zeros(4, 32, 2, H, 32, dtype=BF, device=cuda), pos),  # D
        (qkv, prefix, plen, kv.transpose(1, 2), pos),  # a transposed cache
        (qkv, prefix.transpose(1, 2), plen, kv, pos),
        (qkv, prefix, plen, wide[..., 4:68], pos),  # a misaligned slice: rows start 8 bytes off
        (qkv, prefix, plen, kv, pos.cpu()),  # device
        (qkv, prefix, plen.cpu(), kv, pos),
        (qkv, prefix, plen, kv, pos[:2]),  # counts
        (qkv[0], prefix, plen, kv, pos),  # rank
        (qkv, prefix[0], plen, kv, pos),
        (qkv, prefix, plen.view(2, 1), kv, pos),
    ]
    for i, args in enumerate(bad):
        with pytest.raises(RuntimeError):
            op(*args, 0.125)
            pytest.fail(f"bad argument set {i} was accepted")


def test_inference_only(cuda):
    from replicann_amd import ops as O
    qkv, prefix, kv = C.make(1, 2, H, D, 64, 32, [3], [1, 1], BF, cuda)
    assert torch.is_grad_enabled()
    O.attention_decode_prefix(qkv, prefix, _t([3], cuda), kv, _t([1, 1], cuda))  # the kernels run with grad enabled
    with pytest.raises(RuntimeError, match="inference only"):
        O.attention_decode_prefix(qkv.clone().requires_grad_(), prefix, _t([3], cuda), kv, _t([1, 1], cuda))


def test_schema_and_dispatch_keys(cuda):
    from replicann_amd import _ext
    _ext.ops()
    names = sorted(n for n in torch._C._dispatch_get_all_op_names() if n.startswith("replicann_prefix::"))
    assert names == ["replicann_prefix::attn_decode"]
    assert str(torch.ops.replicann_prefix.attn_decode.default._schema) == (
        "replicann_prefix::attn_decode(Tensor qkv, Tensor prefix_kv, Tensor prefix_len, Tensor(a!) kv, Tensor pos, "
        "float scale) -> Tensor")
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    assert has(names[0], "CUDA")
    assert not any(has(names[0], k) for k in ("CPU", "CompositeExplicitAutograd", "CompositeImplicitAutograd"))


# ------------------------------------------------------------------------------------------------
# 4. the composed path on the GPU
# ------------------------------------------------------------------------------------------------
def test_head_size_32_composed(ops, cuda):
    out, ref, _ = C.run_case(ops.attention_decode_prefix, 3, 5, H, 32, 64, 32, [0, 33, 64],
                             [(5 * b) % 33 for b in range(15)], BF, cuda, seed=6)
    err = C.rel_l2(out, ref)
    print(f"prefix attention D=32 composed: rel L2 {err:.3e}")
    assert err < 1e-2, err


def test_hook_runs_the_composed_path(ops, cuda, monkeypatch):
    from replicann_amd.ops import prefix
    monkeypatch.setattr(prefix, "PREFIX_NATIVE", False)
    op = lambda *a: ops.attention_decode_prefix(*a, takes=False)  # noqa: E731
    out, ref, _ = C.run_case(op, 2, 3, H, D, 64, 32, [20, 64], [0, 5, 32, 31, 1, 7], BF, cuda, seed=7)
    assert C.rel_l2(out, ref) < 1e-2


# ------------------------------------------------------------------------------------------------
# 5. the model
# ------------------------------------------------------------------------------------------------
PLENS, N, NEW = [20, 13], 3, 12


def _model(cuda):
    import replicann_amd as R
    torch.manual_seed(0)
    m = R.GPT2(R.GPT2Config.tiny(n_embd=128, n_head=2, n_layer=2, block_size=128)).to(cuda)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m.eval()


def _prompts(cuda, seed=1):
    idx = torch.randint(0, 1000, (len(PLENS), max(PLENS)), generator=torch.Generator().manual_seed(seed))
    pad = torch.arange(max(PLENS)).unsqueeze(0) >= torch.tensor(PLENS).unsqueeze(1)
    return idx.masked_fill(pad, 0).to(cuda)


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_steps_match_fp32_cpu_model(ops, cuda):
    """Teacher-forced, different forced tokens per sample: the prefill at batch 2, then 12 one-token steps at batch 6,
    eager and captured, every step's logits against the fp32 CPU model run with a plain cache on the repeated prompts."""
    from replicann_amd.models.decoding import KVCache
    m = _model(cuda)
    ref = copy.deepcopy(m).float().cpu().eval()
    idx = _prompts(cuda)
    forced = torch.randint(0, 1000, (6, NEW), generator=torch.Generator().manual_seed(2))
    eager, graph, cpu = KVCache(2, 64, samples=N, tail_len=64), KVCache(2, 64, samples=N, tail_len=64), KVCache(2, 64)
    want = ref.decode_step(idx.cpu().repeat_interleave(N, 0), cpu, lens=[p for p in PLENS for _ in range(N)])
    got = m.decode_step(idx, eager, lens=PLENS)
    assert got.shape[0] == 2 and rel_err(got.repeat_interleave(N, 0), want) < 3e-2
    m.decode_step(idx, graph, lens=PLENS)
    assert eager.prefix[0].shape == (2, 64, 2, 2, 64) and eager.kv[0].shape == (6, 64, 2, 2, 64)
    g, tok, out = m._capture_decode(graph, 6)
    forced_d = forced.to(cuda)
    for t in range(NEW):
        want = ref.decode_step(forced[:, t:t + 1], cpu)
        a = m.decode_step(forced_d[:, t:t + 1], eager)
        tok.copy_(forced_d[:, t:t + 1])
        g.replay()
        ea, eg = rel_err(a, want), rel_err(out, want)
        print(f"shared step {t}: eager {ea:.3e} captured {eg:.3e}")
        assert ea < 3e-2 and eg < 3e-2, t
    torch.cuda.synchronize()
    assert eager.pos_t.tolist() == [NEW] * 6 and graph.pos_t.tolist() == [NEW] * 6
    # the kernels ran: 2 layers x (12 eager steps + the capture's warm-up and recording)
    assert ops.calls == {"attn_decode": 2 * (NEW + 2)}
    for layer in range(2):  # the same tails either way
        assert torch.equal(eager.kv[layer][:, :NEW], graph.kv[layer][:, :NEW])


def test_generate_graph_matches_eager_and_registry(cuda):
    m = _model(cuda)
    fresh = copy.deepcopy(m)
    idx = _prompts(cuda)
    e = m.generate(idx[:, :13], NEW, temperature=0, graph=False, num_samples=N)
    assert len(m._decode_graphs()) == 0
    r = m.generate(idx[:, :13], NEW, temperature=0, graph=True, num_samples=N)
    assert e.shape == (6, 13 + NEW) and torch.equal(e, r)
    assert torch.equal(m.generate(idx[:, :13], NEW, temperature=0, graph=True, num_samples=N), r)  # the stored graph
    keys = list(m._decode_graphs())
    assert len(keys) == 1 and keys[0][-2:] == ("samples", N) and keys[0][:2] == (6, 64)
    assert keys[0][-6:-2] == ("prompts", 2, "tail", 64)
    cache = m._decode_graphs()[keys[0]][0]
    assert cache.prefix[0].shape[0] == 2 and cache.kv[0].shape[0] == 6
    # a plain generate afterwards: a second entry, and the output of a model that never ran a shared step
    a = m.generate(idx[:, :13].repeat_interleave(N, 0), NEW, temperature=0)
    assert len(m._decode_graphs()) == 2
    assert torch.equal(a, fresh.generate(idx[:, :13].repeat_interleave(N, 0), NEW, temperature=0))


def test_generate_ragged_eos(cuda):
    from replicann_amd.ops import rng
    m = _model(cuda)
    idx = _prompts(cuda, seed=3)
    kw = dict(prompt_lens=PLENS, temperature=0.9, top_k=50, sampler="native", num_samples=N)
    rng.manual_seed(7)
    free, fl = m.generate(idx, NEW, graph=False, **kw)
    assert fl.tolist() == [p + NEW for p in PLENS for _ in range(N)]
    eos = int(free[1, PLENS[0] + 1])  # what sample 1 of prompt 0 emits at its second step
    rng.manual_seed(7)
    e, el = m.generate(idx, NEW, graph=False, eos_token_id=eos, **kw)
    # a row's draws depend on the seed stream and its own logits alone: every row is the free run's up to its own EOS
    for b in range(6):
        p, new = PLENS[b // N], free[b, PLENS[b // N]:PLENS[b // N] + NEW].tolist()
        k = new.index(eos) + 1 if eos in new else NEW
        assert int(el[b]) == p + k, b
        assert torch.equal(e[b, :p + k], free[b, :p + k]) and bool((e[b, p + k:] == eos).all())
    assert int(el[1]) <= PLENS[0] + 2 and max(int(el[0]), int(el[2])) > int(el[1])  # its prompt's other samples run on
    # greedy (the samples of a prompt agree, the prompts do not): the captured step against the eager one
    kw = dict(prompt_lens=PLENS, temperature=0, num_samples=N)
    free, _ = m.generate(idx, NEW, graph=False, **kw)
    eos = int(free[0, PLENS[0]])  # prompt 0's samples stop at once
    e, el = m.generate(idx, NEW, graph=False, eos_token_id=eos, **kw)
    r, rl = m.generate(idx, NEW, graph=True, eos_token_id=eos, **kw)
    assert el.tolist()[:N] == [PLENS[0] + 1] * N and torch.equal(el, rl) and torch.equal(e, r)


def test_native_sampler_captured_with_the_shared_step(cuda):
    from replicann_amd.ops import rng
    m = _model(cuda)
    idx = _prompts(cuda)[:, :13]
    kw = dict(temperature=0.9, top_k=50, sampler="native", graph=True, num_samples=N)
    rng.manual_seed(5)
    a = m.generate(idx, NEW, **kw)  # captures
    rng.manual_seed(5)
    b = m.generate(idx, NEW, **kw)  # replays
    rng.manual_seed(6)
    c = m.generate(idx, NEW, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    for g in range(2):  # every sample draws its own tokens
        rows = a[g * N:(g + 1) * N, 13:]
        assert not (torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2]))
    key = next(iter(m._decode_graphs()))
    assert len(m._decode_graphs()) == 1 and "sampler" in key and key[-2:] == ("samples", N)
