"""Speculative sampling on the HIP kernel (csrc/kernels/spec_verify.hip): ``ops.speculative_verify``
against its float64 CPU reference on the same logits and uniforms, its binding, and
``GPT2.generate(draft=..., temperature > 0, sampler="native")`` eager and captured.

Kernel shapes: B = 3; K = 1, 4, 15; V = 1, 7, 8191 (the last size of one bf16 register round is 8192
slots, of which the row start may take 7), 8192·7 + 1 (past the register budget: the re-reading path)
and 50257 (the GPT-2 row: the full register path); bf16 and fp32.  Two layouts: rows cut out of
16-byte aligned, wider buffers (the vector-load path for both rows) and rows of an odd stride starting
at column 3 (no common alignment: the draft row is read element by element in the target row's slots).

Exactness: tokens and ``matched`` must EQUAL the reference except in rows where a decision sits within
rounding of its threshold, which the test finds from the float64 reference: BOUND = 1e-5 (of Z) on
|u_acc · q(d) - p(d)|, on the draw's distance to a CDF edge and on the distance of a top-p decision
(the mass above a tie group against top_p) from its threshold.  The kernel's fp32 error in a
cumulative mass is ~2e-6 of Z (three roundings of the scaled exponent argument, a 1-2 ulp v_exp_f32,
a 59-term sum chain — derived in tests/test_sampling_gpu.py), so the bound holds 5× that.  The
uniforms are chosen on the CPU so that the reference itself stays clear of the bound — acceptance
draws are redrawn away from their threshold, resample / bonus draws sit at the midpoint of the CDF
interval of a token of at least 1e-3 of the mass — and at most 2 % of a case's positions may be
excluded (asserted; on this data none is).

Model tolerances: 3e-2 of the row's largest logit for "among the fp32 model's top 5", as derived in
tests/test_generate_gpu.py.  No acceptance rate is asserted: it is a measurement."""

import copy

import pytest
import torch

from replicann_amd import _ext, ops
from replicann_amd.models import decoding
from replicann_amd.models.decoding import sampler_params
from replicann_amd.ops import rng, sampling, speculative

pytestmark = pytest.mark.gpu

B = 3
BOUND = 1e-5
U_MAX = 1 - 2.0 ** -24
SETTINGS = {"plain": (1.0, None, None), "kp": (0.7, 50, 0.95), "k1": (1.3, 1, None), "greedy": (0.0, None, None)}
# every K with every setting somewhere; the top-p reference (a Python loop over rows) on the smaller windows
PLAN = [(1, "plain"), (1, "kp"), (1, "k1"), (1, "greedy"), (4, "kp"), (4, "plain"), (15, "plain"), (15, "k1"),
        (15, "greedy")]
SCHEMA = ("replicann_spec::verify(Tensor target_logits, Tensor draft_logits, Tensor drafts, float temperature, "
          "int top_k, float top_p, Tensor? u, Tensor? seed_buf, Tensor? params, bool check_drafts) -> (Tensor, Tensor)")
_CASES = {}


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


def _raw():
    _ext.ops()
    return torch.ops.replicann_spec.verify


def _on_device(x, cuda, layout):
    """``x`` (B, R, V) on the device as a view of a wider buffer (a large logit outside the rows)."""
    b, r, V = x.shape
    if layout == "aligned":  # every row start on a 16-byte boundary
        buf = torch.full((b, r, (V + 15) // 8 * 8), 77.0, dtype=x.dtype, device=cuda)
        view = buf[..., :V]
    else:  # an odd row stride, rows from column 3: the row starts take every position against a boundary
        buf = torch.full((b, r + 1, (V + 5) | 1), 77.0, dtype=x.dtype, device=cuda)
        view = buf[:, :r, 3:3 + V]
    view.copy_(x.to(cuda))
    return view


def _top_p_margin(logits, temperature, top_k, top_p):
    """(N,) the distance of the nearest top-p decision of each row from its threshold, in units of Z."""
    out = torch.full((logits.shape[0],), 1.0, dtype=torch.float64)
    if top_p is None or top_p >= 1.0:
        return out
    x = logits.double()
    x = torch.where(x.isnan(), torch.full_like(x, float("-inf")), x)
    _, e = sampling.kept_mask(logits, temperature, top_k, None)
    for n in range(logits.shape[0]):
        vals, inv = torch.unique(x[n], return_inverse=True)
        mass = torch.zeros(vals.numel(), dtype=torch.float64).index_add_(0, inv, e[n])
        greater = mass.flip(0).cumsum(0).flip(0) - mass
        out[n] = (greater[mass > 0] / e[n].sum() - top_p).abs().min()
    return out


def _build(V, dtype, K, name, seed):
    temperature, top_k, top_p = SETTINGS[name]
    g = torch.Generator().manual_seed(seed)
    target = (torch.randn(B, K + 1, V, generator=g) * 3).to(dtype)
    # a draft that resembles its target: accepted and rejected positions both occur
    draft = (target[:, :K].float() + 0.4 * torch.randn(B, K, V, generator=g)).to(dtype)
    # drafts among the draft row's best three: tokens of a probability far above BOUND, as a draft's are
    best = draft.float().topk(min(3, V), dim=-1).indices
    drafts = best.gather(2, torch.randint(0, min(3, V), (B, K, 1), generator=g))[..., 0]
    u = torch.rand(B, K + 1, 2, generator=g)
    amb = torch.zeros(B, K + 1, dtype=torch.bool)
    if temperature > 0:
        p = speculative._probs(target, temperature, top_k, top_p)
        q = speculative._probs(draft, temperature, top_k, top_p)
        at = drafts.unsqueeze(-1)
        pd, qd = p[:, :K].gather(2, at)[..., 0], q.gather(2, at)[..., 0]
        for _ in range(4):  # acceptance draws away from their threshold
            near = (u[:, :K, 0].double() * qd - pd).abs() < 10 * BOUND
            u[:, :K, 0] = torch.where(near, torch.rand(B, K, generator=g), u[:, :K, 0])
        res = (p[:, :K] - q).clamp(min=0)
        res = torch.where(res.sum(-1, keepdim=True) > 0, res, p[:, :K])
        w = torch.cat([res, p[:, K:]], 1)
        w = w / w.sum(-1, keepdim=True)
        cdf = w.cumsum(-1)
        first = (cdf > u[..., 1:].double()).to(torch.int8).argmax(-1, keepdim=True)  # the token a free draw would take
        tok = torch.where(w.gather(2, first) >= 1e-3, first, w.argmax(-1, keepdim=True))
        u[..., 1] = (cdf.gather(2, tok) - w.gather(2, tok) / 2)[..., 0].float().clamp(0, U_MAX)  # mid-interval
        ud = u[..., 1:].double()
        acc_amb = ((u[:, :K, 0].double() * qd - pd).abs() < BOUND) & (qd > 0)
        draw_amb = torch.minimum((cdf - ud).abs().min(-1).values, ud[..., 0]) < BOUND
        flt_t = _top_p_margin(target.reshape(-1, V), temperature, top_k, top_p).view(B, K + 1) < BOUND
        flt_d = _top_p_margin(draft.reshape(-1, V), temperature, top_k, top_p).view(B, K) < BOUND
        amb = draw_amb | flt_t
        amb[:, :K] |= acc_amb | flt_d
    return target, draft, drafts, u, amb


def _case(V, dtype, K, name):
    """Host data of one case, made once and never changed: logits, drafts, uniforms, the reference's
    (tokens, matched) and the rows that hold a decision within BOUND of its threshold.  The data come
    from the first of a few fixed seeds that keeps the reference under the 2 % cap (a condition on the
    inputs, decided on the CPU before any kernel runs)."""
    key = (V, dtype, K, name)
    if key in _CASES:
        return _CASES[key]
    for attempt in range(6):
        target, draft, drafts, u, amb = _build(V, dtype, K, name, 100 * V + 10 * K + len(name) + 7919 * attempt)
        if int(amb.sum()) <= 0.02 * B * (K + 1):
            break
    assert int(amb.sum()) <= 0.02 * B * (K + 1), f"{int(amb.sum())} of {B * (K + 1)} positions within {BOUND} of a threshold"
    tokens, matched = speculative.reference(target, draft, drafts, *SETTINGS[name], u)
    # a row is compared exactly unless a position up to its first rejection is within BOUND of a threshold
    j = torch.arange(K + 1).view(1, K + 1)
    skip = (amb & (j <= matched.view(B, 1))).any(1)
    _CASES[key] = (target, draft, drafts, u, tokens, matched, skip)
    return _CASES[key]


def _twice(*a, **kw):
    """The kernel's (tokens, matched) on the CPU, after checking that a second run is bit-equal."""
    t1, m1 = ops.speculative_verify(*a, **kw)
    t2, m2 = ops.speculative_verify(*a, **kw)
    assert t1.dtype == torch.int64 and m1.dtype == torch.int64
    assert torch.equal(t1, t2) and torch.equal(m1, m2)
    return t1.cpu(), m1.cpu()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1, 7, 8191, 8192 * 7 + 1, 50257])
def test_kernel_matches_reference(cuda, V, dtype):
    for K, name in PLAN:
        target, draft, drafts, u, tokens, matched, skip = _case(V, dtype, K, name)
        temperature, top_k, top_p = SETTINGS[name]
        for layout in ("aligned", "odd"):
            tok, m = _twice(_on_device(target, cuda, layout), _on_device(draft, cuda, layout), drafts.to(cuda),
                            temperature, top_k, top_p, u=u.to(cuda))
            assert tok.shape == (B, K + 1) and m.shape == (B,)
            assert int(tok.min()) >= 0 and int(tok.max()) < V and int(m.min()) >= 0 and int(m.max()) <= K
            for b in range(B):
                a = int(m[b])
                assert tok[b, :a].tolist() == drafts[b, :a].tolist() and bool((tok[b, a + 1:] == 0).all()), (K, name, b)
                if not bool(skip[b]):
                    assert a == int(matched[b]) and tok[b].tolist() == tokens[b].tolist(), (K, name, layout, b)


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 50257), (torch.float32, 8191), (torch.bfloat16, 8192 * 7 + 1)],
                         ids=["bf16-50257", "fp32-8191", "bf16-57345"])
def test_equal_rows_accept_every_draft_for_every_u(cuda, dtype, V):
    K = 4
    target = _case(V, dtype, K, "kp")[0]
    best = target[:, :K].float().topk(2, dim=-1).indices
    for name in ("plain", "kp"):
        # drafts of non-zero probability: the best token, at odd positions the second best where the filters keep it
        keep = sampling.kept_mask(target[:, :K].reshape(B * K, V), *SETTINGS[name])[0].view(B, K, V)
        second = torch.where(keep.gather(2, best[..., 1:])[..., 0], best[..., 1], best[..., 0])
        drafts = torch.where(torch.arange(K) % 2 == 1, second, best[..., 0])
        for ua in (0.0, 0.5, U_MAX, 1.0):  # 1.0: clamped to the largest uniform below 1
            u = torch.full((B, K + 1, 2), 0.5)
            u[..., 0] = ua
            for layout in ("aligned", "odd"):
                t = _on_device(target, cuda, layout)
                d = _on_device(target[:, :K], cuda, layout)
                tok, m = _twice(t, d, drafts.to(cuda), *SETTINGS[name], u=u.to(cuda))
                assert m.tolist() == [K] * B and torch.equal(tok[:, :K], drafts), (name, ua, layout)
                bonus = ops.sample_logits(t[:, K], *SETTINGS[name], u=u[:, K, 1].contiguous().to(cuda))[0].cpu()
                assert torch.equal(tok[:, K:], bonus)  # the bonus token is the sampler's own draw from p_K


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_draft_at_a_masked_target_logit_is_rejected_and_never_returned(cuda, dtype):
    K, V = 4, 50257
    target, draft, drafts, u = (t.clone() for t in _case(V, dtype, K, "plain")[:4])
    for b in range(B):
        for i in range(K):
            target[b, i, drafts[b, i]] = float("nan") if (b + i) % 2 else float("-inf")
    u[..., 0] = 0.0  # the most accepting draw
    for name in ("plain", "kp"):
        tok, m = _twice(_on_device(target, cuda, "aligned"), _on_device(draft, cuda, "aligned"), drafts.to(cuda),
                        *SETTINGS[name], u=u.to(cuda))
        assert m.tolist() == [0] * B and bool((tok[:, 1:] == 0).all())
        for b in range(B):
            assert int(tok[b, 0]) != int(drafts[b, 0]) and bool(torch.isfinite(target[b, 0, tok[b, 0]].float()))


def test_seed_buf_draws_are_hash_uniform(cuda):
    K, V = 4, 50257
    target, draft, drafts = _case(V, torch.bfloat16, K, "kp")[:3]
    t, d, dr = _on_device(target, cuda, "aligned"), _on_device(draft, cuda, "aligned"), drafts.to(cuda)
    rng.manual_seed(11)
    seed = rng.next_seed(cuda)
    tok, m = _twice(t, d, dr, *SETTINGS["kp"], seed_buf=seed)
    s = int(seed.cpu()) & ((1 << 64) - 1)
    u = torch.tensor([sampling.hash_uniform(s, n) for n in range(2 * B * (K + 1))], dtype=torch.float32)
    tok2, m2 = _twice(t, d, dr, *SETTINGS["kp"], u=u.view(B, K + 1, 2).to(cuda))
    assert torch.equal(tok, tok2) and torch.equal(m, m2)


def test_params_override_the_host_settings(cuda):
    K, V = 4, 8191
    target, draft, drafts, u = _case(V, torch.bfloat16, K, "kp")[:4]
    t, d, dr = _on_device(target, cuda, "aligned"), _on_device(draft, cuda, "aligned"), drafts.to(cuda)
    outs = []
    for name in ("kp", "plain", "k1", "greedy"):
        want = _twice(t, d, dr, *SETTINGS[name], u=u.to(cuda))
        got = _twice(t, d, dr, 1.0, 7, 0.5, u=u.to(cuda), params=sampler_params(*SETTINGS[name], device=cuda))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
        outs.append(want[0])
    assert not all(torch.equal(outs[0], o) for o in outs[1:])  # the settings matter on this data


def test_binding_checks(cuda):
    op = _raw()
    K, V = 2, 64
    t = torch.zeros(B, K + 1, V, dtype=torch.bfloat16, device=cuda)
    d = torch.zeros(B, K, V, dtype=torch.bfloat16, device=cuda)
    dr = torch.zeros(B, K, dtype=torch.long, device=cuda)
    u = torch.zeros(B, K + 1, 2, device=cuda)
    seed = torch.zeros(1, dtype=torch.long, device=cuda)
    par = torch.tensor([1.0, 0.0, 1.0], device=cuda)
    assert op(t, d, dr, 1.0, 0, 1.0, u, None, None, True)[0].shape == (B, K + 1)
    assert op(t, d, dr, 1.0, 0, 1.0, None, seed, par, True)[1].tolist() == [K] * B  # equal rows: all accepted
    assert op(t, d, dr + V, 1.0, 0, 1.0, u, None, None, False)[1].tolist() == [0] * B  # unchecked: rejected on the device
    z = lambda *s, **kw: torch.zeros(*s, device=cuda, **{"dtype": torch.bfloat16, **kw})  # noqa: E731
    bad = [
        (z(B, 1, V), z(B, 0, V), torch.zeros(B, 0, dtype=torch.long, device=cuda), u[:, :1], None),  # K = 0
        (z(B, 17, V), z(B, 16, V), torch.zeros(B, 16, dtype=torch.long, device=cuda), z(B, 17, 2, dtype=torch.float32), None),
        (t, d.float(), dr, u, None), (t.half(), d.half(), dr, u, None),  # dtypes
        (t, d, dr.int(), u, None),
        (z(B, K + 1, 2 * V)[..., ::2], d, dr, u, None), (t, z(B, K, 2 * V)[..., ::2], dr, u, None),  # last stride
        (t.transpose(0, 1)[:, :, :], d, dr, u, None),
        (t, d, dr + V, u, None), (t, d, dr - 1, u, None),  # drafts out of [0, V)
        (t, d[:, :1], dr, u, None), (t, d[..., :32], dr, u, None), (t, d, dr[:, :1], u, None), (t[0], d[0], dr[0], u[0], None),
        (t.cpu(), d, dr, u, None), (t, d.cpu(), dr, u, None), (t, d, dr.cpu(), u, None), (t, d, dr, u.cpu(), None),  # devices
        (t, d, dr, None, seed.cpu()),
        (t, d, dr, None, None), (t, d, dr, u, seed),  # exactly one of u and seed_buf
        (t, d, dr, u[..., :1], None), (t, d, dr, u.double(), None),
    ]
    for a in bad:
        with pytest.raises(RuntimeError):
            op(*a[:3], 1.0, 0, 1.0, a[3], a[4], None, True)
    for kw in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5)):
        a = dict(temperature=1.0, top_k=0, top_p=1.0)
        a.update(kw)
        with pytest.raises(RuntimeError):
            op(t, d, dr, a["temperature"], a["top_k"], a["top_p"], u, None, None, True)
    for p in (par.cpu(), par[:2], par.double()):
        with pytest.raises(RuntimeError):
            op(t, d, dr, 1.0, 0, 1.0, u, None, p, True)


def test_schema_and_dispatch_key_are_pinned():
    op = _raw()
    assert str(op.default._schema) == SCHEMA
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    assert has("replicann_spec::verify", "CUDA")
    assert not any(has("replicann_spec::verify", k) for k in ("CPU", "CompositeExplicitAutograd",
                                                             "CompositeImplicitAutograd"))
    assert [n for n in torch._C._dispatch_get_all_op_names() if n.startswith("replicann_spec::")] == [
        "replicann_spec::verify"]


# ------------------------------------------------------------------ the model
PLENS = [5, 20, 13]
NEW = 12


def _model(cuda, n_head, seed=0):
    import replicann_amd as R
    torch.manual_seed(seed)
    m = R.GPT2(R.GPT2Config.tiny(n_embd=128, n_head=n_head, n_layer=2, block_size=128)).to(cuda)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m.eval()


def _padded(cuda, seed=1, junk=False):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, 1000, (len(PLENS), max(PLENS)), generator=g)
    pad = torch.arange(max(PLENS)).unsqueeze(0) >= torch.tensor(PLENS).unsqueeze(1)
    fill = torch.randint(0, 1000, idx.shape, generator=g) if junk else torch.zeros_like(idx)
    return torch.where(pad, fill, idx).to(cuda)


def _assert_top5(ref, tokens, lens, margin=3e-2):
    for b, p in enumerate(PLENS):
        row = tokens[b, : int(lens[b])].cpu()
        with torch.no_grad():
            full = ref(row.unsqueeze(0))[0]
        for t in range(p, int(lens[b])):
            lg = full[t - 1]
            assert lg[row[t]] >= lg.topk(5).values[-1] - margin * lg.abs().max(), (b, t)


@pytest.mark.parametrize("n_head", [2, 4])
@pytest.mark.parametrize("which", ["same", "other"])
def test_generate_with_draft_sampling_gpu(cuda, n_head, which):
    m = _model(cuda, n_head)
    draft = m if which == "same" else _model(cuda, n_head, seed=7)
    ref = copy.deepcopy(m).float().cpu().eval()
    idx = _padded(cuda)
    kw = dict(prompt_lens=PLENS, temperature=0.8, top_k=5, sampler="native", draft=draft, draft_k=4)
    # an untested first call: the GEMM autotuner settles each decode shape's kernel during it, so the
    # exact-equality comparisons below are between runs on the same kernels
    m.generate(idx, NEW, graph=False, **kw)
    runs = {}
    for graph in (True, False):
        rng.manual_seed(5)
        stats = {}
        tokens, lens = m.generate(idx, NEW, graph=graph, stats=stats, **kw)
        assert lens.tolist() == [p + NEW for p in PLENS] and tokens.shape == (3, max(PLENS) + NEW)
        for b, p in enumerate(PLENS):
            assert torch.equal(tokens[b, :p], idx[b, :p])
            assert bool((tokens[b, p + NEW:] == 0).all())
        _assert_top5(ref, tokens, lens)  # every committed token, whichever model proposed it
        assert 1 <= stats["rounds"] <= NEW - 1
        assert all(0 <= a <= d for a, d in zip(stats["accepted"].tolist(), stats["drafted"].tolist()))
        runs[graph] = tokens
    assert torch.equal(runs[True], runs[False])  # the same seeds: the same draws, captured or not
    rng.manual_seed(5)
    junk, _ = m.generate(_padded(cuda, junk=True), NEW, graph=True, **kw)
    assert torch.equal(junk, runs[True])  # whatever the padding holds
    rng.manual_seed(6)
    other_seed, _ = m.generate(idx, NEW, graph=True, **kw)
    assert not torch.equal(other_seed, runs[True])  # sampling is on: another seed, another text
    # an EOS taken from the run: each row equals it up to and including its first EOS, pad after
    eos = int(runs[True][1, PLENS[1] + 3])
    rng.manual_seed(5)
    got, glens = m.generate(idx, NEW, graph=True, eos_token_id=eos, pad_token_id=0, **kw)
    for b, p in enumerate(PLENS):
        gen = runs[True][b, p: p + NEW].tolist()
        n = gen.index(eos) + 1 if eos in gen else NEW
        assert int(glens[b]) == p + n, b
        assert got[b, : p + n].tolist() == runs[True][b, : p + n].tolist(), b
        assert bool((got[b, p + n:] == 0).all()), b
    assert int(glens[1]) <= PLENS[1] + 4
    # top_k = 1 leaves the arg-maxes: the greedy speculative output
    greedy, _ = m.generate(idx, NEW, graph=True, prompt_lens=PLENS, temperature=0, draft=draft, draft_k=4)
    top1, _ = m.generate(idx, NEW, graph=True, **{**kw, "top_k": 1})
    assert torch.equal(top1, greedy)
    # uniform call: a plain tensor
    uni = m.generate(idx[:, :5], NEW, draft=draft, draft_k=2, temperature=0.8, top_k=5, sampler="native")
    assert torch.is_tensor(uni) and uni.shape == (3, 5 + NEW)
    for mm in {m, draft}:
        assert len(mm._decode_graphs()) <= decoding.DECODE_GRAPHS_MAX
    assert any("window" in k and "logits" in k for k in m._decode_graphs())
