"""The fused sampler kernel (``csrc/kernels/sampling.hip``) against the float64 CPU reference of the
same semantics (``ops.sample_logits`` on CPU tensors, ``ops/sampling.py``) on the same logits.

Shapes: V = 1, 33, 1025 (one register round; rows cut out of a wider buffer at column 1, odd row
strides: no row start is 16-byte aligned), 50257 (the GPT-2 row, ``[:, :50257]`` of a 50304-wide
buffer: the full register path) and 57400 (past the register budget: the re-reading path); B = 1, 3
and one B = 64 call; bf16 and fp32.

EPS = 2e-5 bounds the kernel's relative error in a cumulative mass.  It is derived, not measured:
fp32 rounding of the scaled exponent argument of the terms that carry mass (|x - max| <~ 10, three
roundings) ~ 2e-6, a 1-2 ulp v_exp_f32 1.2e-7, at worst a 59-term fp32 sum chain 3.5e-6; times 3.
``kept`` and tokens are compared EXACTLY wherever the float64 reference is at least 10 EPS away
from a decision boundary — top_p is picked from the data so that it is (a condition on the inputs,
asserted on the CPU) — and every token must lie in its float64 CDF interval widened by EPS."""

import pytest
import torch

from replicann_amd import ops
from replicann_amd.ops import rng, sampling

pytestmark = pytest.mark.gpu

EPS = 2e-5
U_MAX = 1 - 2.0 ** -24
INF = float("inf")
WIDTH = {1: 3, 33: 37, 1025: 1031, 50257: 50304, 57400: 57405}
SETTINGS = [  # (temperature, top_k, nominal top_p)
    (1.0, None, None), (1.0, 1, None), (1.0, 5, None), (1.0, 50, None), (1.0, 1 << 20, None),
    (1.0, None, 1.0), (1.0, None, 0.9), (0.7, 40, 0.95),
    (1.0, 2000, None),  # more than one key per thread can decide: the select runs all its passes over the row
]
_ROWS = {}


def _rows(V, dtype):
    """(3, V) seeded N(0, 3²) logits in ``dtype`` on the CPU, made once per (V, dtype) and shared."""
    if (V, dtype) not in _ROWS:
        g = torch.Generator().manual_seed(1000 + V)
        _ROWS[V, dtype] = (torch.randn(3, V, generator=g) * 3).to(dtype)
    return _ROWS[V, dtype]


def _on_device(x, cuda):
    """``x`` (B, V) as a column slice of a wider device buffer (see the module docstring)."""
    B, V = x.shape
    c0 = 0 if V == 50257 else 1
    buf = torch.full((B, WIDTH[V]), 77.0, dtype=x.dtype, device=cuda)  # a large logit outside the row
    buf[:, c0:c0 + V] = x.to(cuda)
    return buf[:, c0:c0 + V]


def _pick_top_p(row, temperature, top_k, nominal):
    """top_p from the data: the midpoint between two adjacent tie-group boundaries of the float64
    cumulative mass, at least 10 EPS from both, nearest ``nominal``."""
    if nominal is None or nominal >= 1.0:
        return nominal
    _, e = sampling.kept_mask(row, temperature, top_k, None)
    x = row[0].double()
    vals, inv = torch.unique(x, return_inverse=True)
    mass = torch.zeros(vals.numel(), dtype=torch.float64).index_add_(0, inv, e[0]).flip(0)  # descending logits
    bounds = torch.cat([torch.zeros(1, dtype=torch.float64), mass[mass > 0].cumsum(0)]) / e.sum()
    mid, half = (bounds[1:] + bounds[:-1]) / 2, (bounds[1:] - bounds[:-1]) / 2
    ok = (half >= 10 * EPS) & (mid < 1.0)
    assert bool(ok.any()), "no top_p with a 10 EPS margin on this row: change its seed"
    p = float(mid[ok][(mid[ok] - nominal).abs().argmin()])
    assert min(abs(p - float(b)) for b in bounds) >= 10 * EPS
    return p


def _twice(logits, *a, **kw):
    """The kernel's (tokens, kept) on the CPU, after checking that a second run is bit-equal."""
    t1, k1 = ops.sample_logits(logits, *a, **kw)
    t2, k2 = ops.sample_logits(logits, *a, **kw)
    assert t1.shape == (logits.shape[0], 1) and t1.dtype == torch.int64 and k1.dtype == torch.int32
    assert torch.equal(t1, t2) and torch.equal(k1, k2)
    return t1.cpu(), k1.cpu()


def _check(x, cuda, temperature, top_k, top_p, u):
    """One launch on ``x`` (B, V; CPU) against the reference: ``kept`` exact, every token kept and inside its
    float64 CDF interval widened by EPS."""
    tok, kept = _twice(_on_device(x, cuda), temperature, top_k, top_p, u=u.to(cuda))
    keep, e = sampling.kept_mask(x, temperature, top_k, top_p)
    assert torch.equal(kept, keep.sum(-1).to(torch.int32)), (kept, keep.sum(-1))
    V = x.shape[1]
    assert int(tok.min()) >= 0 and int(tok.max()) < V
    cdf, Z = e.cumsum(-1), e.sum(-1)
    for b in range(x.shape[0]):
        i = int(tok[b])
        assert bool(keep[b, i]) and float(e[b, i]) > 0, (b, i)
        lo = float(cdf[b, i - 1]) if i else 0.0
        t, z = float(u[b].double() * Z[b]), float(Z[b])
        assert lo - EPS * z <= t <= float(cdf[b, i]) + EPS * z, (b, i, lo / z, t / z, float(cdf[b, i]) / z)
    return keep, e


def _check_exact_tokens(row, cuda, temperature, top_k, top_p, keep, e, n_rows=None):
    """The row repeated with u at the midpoints of its float64 CDF intervals (those at least 10 EPS
    from both ends): the tokens must equal the reference's."""
    p = e[0] / e[0].sum()
    cdf = p.cumsum(0)
    idx = torch.nonzero(p / 2 >= 10 * EPS).flatten()
    assert idx.numel() >= 1
    u = (cdf[idx] - p[idx] / 2).float()
    want = idx
    if n_rows is not None:  # fill the batch with further uniforms, each at least 10 EPS from every boundary
        g = torch.Generator().manual_seed(7)
        extra = torch.rand(4 * n_rows, generator=g)
        far = ((extra.double().unsqueeze(1) - cdf[keep[0]].unsqueeze(0)).abs().min(1).values >= 10 * EPS)
        extra = extra[far][: n_rows - idx.numel()]
        assert idx.numel() + extra.numel() == n_rows
        u = torch.cat([u, extra])
        want = (cdf.unsqueeze(0) > u.double().unsqueeze(1)).to(torch.int8).argmax(1)  # the first index past u
    x = row.expand(u.numel(), -1).contiguous()
    tok, kept = _twice(_on_device(x, cuda), temperature, top_k, top_p, u=u.to(cuda))
    assert torch.equal(tok.flatten(), want)
    assert bool((kept == int(keep.sum())).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [1, 33, 1025, 50257, 57400])
def test_kernel_matches_reference(cuda, V, dtype):
    rows = _rows(V, dtype)
    u3 = torch.rand(3, generator=torch.Generator().manual_seed(V))
    for temperature, top_k, nominal in SETTINGS:
        if nominal is None or nominal >= 1.0:  # one launch per batch size
            _check(rows, cuda, temperature, top_k, nominal, u3)
            keep, e = _check(rows[:1], cuda, temperature, top_k, nominal, u3[:1])
            top_p = nominal
        else:  # top_p comes from each row's own data: a launch per row (B = 1 at three row offsets)
            for b in (2, 1, 0):
                top_p = _pick_top_p(rows[b:b + 1], temperature, top_k, nominal)
                keep, e = _check(rows[b:b + 1], cuda, temperature, top_k, top_p, u3[b:b + 1])
        if int(keep.sum()) <= 64:
            _check_exact_tokens(rows[:1], cuda, temperature, top_k, top_p, keep, e)


def test_batch_of_64_same_row(cuda):
    """The GPT-2 row in all 64 rows of one launch (top_k 40, top_p ~ 0.95, temperature 0.7) with 64
    different uniforms: every kept token's CDF midpoint, the rest random."""
    row = _rows(50257, torch.bfloat16)[:1]
    top_p = _pick_top_p(row, 0.7, 40, 0.95)
    keep, e = sampling.kept_mask(row, 0.7, 40, top_p)
    assert int(keep.sum()) <= 64
    _check_exact_tokens(row, cuda, 0.7, 40, top_p, keep, e, n_rows=64)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_extremes(cuda, dtype):
    def run(x, u, temperature=1.0, top_k=None, top_p=None):
        x = x.to(dtype)
        tok, kept = _twice(_on_device(x, cuda), temperature, top_k, top_p, u=torch.tensor(u, device=cuda))
        want = ops.sample_logits(x, temperature, top_k, top_p, u=torch.tensor(u))
        assert torch.equal(tok, want[0]) and torch.equal(kept, want[1])
        return tok.flatten().tolist(), kept.tolist()

    x = torch.cat([torch.tensor([[-INF, 0.5, -INF, 2.0, 1.0, -INF]] * 3), torch.full((3, 27), -INF)], 1)  # V = 33
    assert run(x, [0.0, U_MAX, 0.5]) == ([1, 4, 3], [33, 33, 33])  # first / last token of non-zero mass
    assert run(x, [0.0, U_MAX, 0.5], 0.0) == ([3, 3, 3], [1, 1, 1])  # greedy
    ties = torch.tensor([[1.0, 7.0, 7.0, -2.0, 7.0]]).repeat(3, 1)
    ties = torch.cat([ties, torch.full((3, 1020), -5.0)], 1)  # V = 1025
    assert run(ties, [0.1, 0.5, 0.9], 0.0)[0] == [1, 1, 1]  # lowest index on ties
    assert run(ties, [0.0, 0.5, U_MAX], 1.0, 2) == ([1, 2, 4], [3, 3, 3])  # the whole tie group at the k-th value
    for V in (33, 50257):  # an all-equal row is one tie group: every filter keeps all of it
        eq = torch.full((3, V), 0.25)
        for top_k, top_p in [(None, None), (5, None), (None, 0.3), (5, 0.3)]:
            assert run(eq, [0.0, U_MAX, 0.5], 0.8, top_k, top_p) == ([0, V - 1, V // 2], [V, V, V])
    for V in (33, 1025, 50257):  # all -inf but one
        one = torch.full((3, V), -INF)
        one[:, V // 3] = -3.0
        assert run(one, [0.0, U_MAX, 0.5])[0] == [V // 3] * 3
        assert run(one, [0.0, U_MAX, 0.5], 0.5, 3, 0.5) == ([V // 3] * 3, [1, 1, 1])
        assert run(one, [0.0, U_MAX, 0.5], 0.0)[0] == [V // 3] * 3
    nan = _rows(1025, dtype).clone().float()
    nan[:, ::7] = float("nan")  # unspecified beyond: a valid index
    tok, _ = ops.sample_logits(_on_device(nan.to(dtype), cuda), 1.0, 5, 0.9, u=torch.rand(3, device=cuda))
    assert int(tok.min()) >= 0 and int(tok.max()) < 1025


def test_seed_path(cuda):
    x = _on_device(_rows(50257, torch.bfloat16), cuda)
    rng.manual_seed(5)
    s1 = rng.next_seed(cuda)
    s2 = rng.next_seed(cuda)
    rng.manual_seed(5)
    s3 = rng.next_seed(cuda)
    assert int(s1) == int(s3) and int(s1) != int(s2)  # same state, same draw; consecutive draws differ
    a = ops.sample_logits(x, 0.9, 50, 0.95, seed_buf=s1)
    b = ops.sample_logits(x, 0.9, 50, 0.95, seed_buf=s3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    u = torch.tensor([sampling.hash_uniform(int(s1) & (2 ** 64 - 1), b) for b in range(3)], device=cuda)
    c = ops.sample_logits(x, 0.9, 50, 0.95, u=u)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    xs = x[:1].expand(64, -1).contiguous()  # 64 rows draw 64 different uniforms from one seed
    assert ops.sample_logits(xs, 1.0, seed_buf=s2)[0].unique().numel() > 8


def test_params_tensor(cuda):
    x = _on_device(_rows(1025, torch.float32), cuda)
    u = torch.tensor([0.2, 0.5, 0.8], device=cuda)
    params = torch.tensor([0.7, 5.0, 1.0], device=cuda)
    a = ops.sample_logits(x, 0.7, 5, None, u=u)
    b = ops.sample_logits(x, u=u, params=params)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and b[1].tolist() == [5, 5, 5]
    params.copy_(torch.tensor([1.3, 0.0, 1.0]))  # the same call: the filter read from the device changes
    c = ops.sample_logits(x, u=u, params=params)
    d = ops.sample_logits(x, 1.3, None, None, u=u)
    assert torch.equal(c[0], d[0]) and c[1].tolist() == [1025] * 3
    params.copy_(torch.tensor([0.0, 0.0, 1.0]))
    assert torch.equal(ops.sample_logits(x, u=u, params=params)[0].flatten(), x.argmax(-1))


def test_argument_checks(cuda):
    x = torch.randn(2, 40, device=cuda)
    u = torch.rand(2, device=cuda)
    op = torch.ops.replicann.sample_logits
    for bad in [
        lambda: op(x, 1.0, 0, 1.0, None, None, None),  # neither u nor seed_buf
        lambda: op(x, 1.0, 0, 1.0, u, torch.zeros(1, dtype=torch.long, device=cuda), None),  # both
        lambda: op(x, 1.0, 0, 0.0, u, None, None),  # top_p outside (0, 1]
        lambda: op(x, -1.0, 0, 1.0, u, None, None),
        lambda: op(x, 1.0, -1, 1.0, u, None, None),
        lambda: op(x.half(), 1.0, 0, 1.0, u, None, None),  # dtype
        lambda: op(x.t(), 1.0, 0, 1.0, u, None, None),  # column stride
        lambda: op(x, 1.0, 0, 1.0, u[:1], None, None),  # one uniform per row
        lambda: op(x, 1.0, 0, 1.0, u.cpu(), None, None),  # device
        lambda: op(x, 1.0, 0, 1.0, u, None, torch.ones(2, device=cuda)),  # params: 3 values
        lambda: op(x, 1.0, 0, 1.0, u.double(), None, None),
    ]:
        with pytest.raises(RuntimeError):
            bad()
