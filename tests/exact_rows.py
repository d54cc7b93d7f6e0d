"""Every-element checks of the row kernels: LayerNorm, softmax / cross-entropy, the embedding, and the column
reductions behind them (csrc/kernels/layernorm.hip, softmax_xent.hip, embedding_optim.hip, common.h).

The generators, float64 references, bounds and case functions, in the manner of tests/exact_ints.py.  A whole-
tensor norm does not move for one wrong row, one wrong 8-element chunk or one column left out of a mean, and
those are the mistakes a grid-stride row walk with a prefetch, a ``c < nvec`` guard on a partial chunk, a
chunk that straddles ``n_valid``, per-thread local maxima, an owner table or a ticketed last-block reduction
can make.  So every comparison here is per element:

  bitwise   where the result is exactly computable (integer gradients summed in fp32, one rounding of an
            exact fp32 sum): ``exact_ints.bitwise_report``;
  bounded   elsewhere: |got - float64| <= a bound derived in the case's docstring from the number formats and
            the depth of each reduction (u = 2^-24 is the fp32 unit roundoff, 2^-8 the bf16 one).  A failure
            reports how many elements missed, the first and the worst (``bound_report``); the largest
            error / bound ratio of each check is kept in ``RATIOS`` (profiles/row_kernels_parity.txt).

All references are float64 and computed from the same bf16 inputs the kernel sees.

The cases run on either device.  On CUDA tensors the backend is the raw ops (``torch.ops.replicann``), one stage
at a time rather than through autograd (tests/test_rows_exact_gpu.py).  On CPU tensors it is ``Emu``, an fp32
torch emulation of each op, which checks every generator, precondition, reference and bound without a GPU; with
a ``slip`` it is deliberately wrong in one way a kernel could be, and the CPU tier asserts that the case fails
while the whole-tensor ``rel_err < 1e-2`` of tests/test_ops_gpu.py still passes (tests/test_exact_rows.py).
A plain module, not a conftest.
"""

import functools
import math

import torch

from exact_ints import (BF16_EXACT_INT, F32_EXACT_INT, SENTINEL, Misses, expect_bf16, gen, int_operand,
                        require_representable)

U = 2.0**-24  # fp32 unit roundoff
BF = 2.0**-8  # bf16 unit roundoff: 8 significand bits, so round-to-nearest is off by at most half of 2^-7 relative
# (1 + 2^-8 is a tie between 1 and 1 + 2^-7).  The issue that asked for these checks wrote 2^-9 for "the one bf16
# rounding"; no correct rounding can meet that (exact_ints.gelu_report has it right), so every bound here carries 2^-8.
EPS = 1e-5
INF = float("inf")
L2E = 1.4426950408889634

RATIOS = {}  # "case: check" -> the largest error / bound ratio seen (bounded checks only)
LAST = {}  # name -> (output, float64 reference) of the last case run, for the whole-tensor metric of the CPU tier


def rel_err(a, b):
    """The whole-tensor metric of tests/test_ops_gpu.py, which these checks replace: blind to local errors."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------
# the comparison
# ------------------------------------------------------------------------------------------------
def _as2d(t):
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def bound_report(got, ref64, bound64):
    """(None or the report of the elements with |got - ref| > bound or a non-finite value, the largest
    error / bound ratio).  Per element: one wrong element fails."""
    got, ref64, bound64 = _as2d(got), _as2d(ref64), _as2d(bound64)
    assert got.shape == ref64.shape == bound64.shape, (tuple(got.shape), tuple(ref64.shape), tuple(bound64.shape))
    assert ref64.dtype == torch.float64 and bool(torch.isfinite(ref64).all()) and bool((bound64 >= 0).all())
    g64 = got.double()
    err = (g64 - ref64).abs()
    err = torch.where(torch.isfinite(g64), err, torch.full_like(err, INF))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound64)  # 0 / 0 is a hit, x / 0 a miss
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = ~(err <= bound64)
    n = int(bad.sum())
    if n == 0:
        return None, worst
    r, c = (int(v) for v in bad.nonzero()[0])
    w = int(ratio.argmax())
    wr, wc = w // got.shape[1], w % got.shape[1]

    def at(i, j):
        return (f"({i}, {j}): got {float(got[i, j])!r}, float64 {float(ref64[i, j])!r}, bound "
                f"{float(bound64[i, j]):.3e}")

    return (f"{n} of {bad.numel()} elements over the bound; first at {at(r, c)}; worst at {at(wr, wc)}, "
            f"error / bound {worst:.3g}"), worst


class Checks(Misses):
    """The misses of one case, bitwise (``check``) and bounded (``bound``); ``done`` names all of them."""

    def __init__(self, label, zero_sign=True):
        super().__init__(zero_sign)
        self.label = label

    def bound(self, what, got, ref64, bound64):
        rep, worst = bound_report(got, ref64, bound64)
        key = f"{self.label}: {what}"
        RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
        if rep is not None:
            self.reports.append(f"[{what}] {rep}")

    def zeros(self, what, t):
        """Every element exactly zero (either sign)."""
        t = _as2d(t)
        bad = t != 0
        n = int(bad.sum())
        if n:
            r, c = (int(v) for v in bad.nonzero()[0])
            self.reports.append(f"[{what}] {n} of {bad.numel()} elements are not exactly zero; first at ({r}, {c}): "
                                f"{float(t[r, c])!r}")

    def done(self):
        assert not self.reports, f"{self.label}: {len(self.reports)} check(s) failed:\n" + "\n\n".join(self.reports)


def sentinel_rows(x, before=3, after=5):
    """(big, view): ``x`` copied into rows [before, before + M) of a larger sentinel-filled buffer."""
    big = torch.full((before + x.shape[0] + after, x.shape[1]), SENTINEL, device=x.device, dtype=x.dtype)
    view = big[before:before + x.shape[0]]
    view.copy_(x)
    assert view.is_contiguous()
    return big, view


def rows_untouched(big, x, before=3):
    M = x.shape[0]
    return (bool((big[:before] == SENTINEL).all()) and bool((big[before + M:] == SENTINEL).all())
            and bool((big[before:before + M] == x).all()))


# ------------------------------------------------------------------------------------------------
# the ops under test: the HIP kernels, or their fp32 emulation (with a slip: wrong in one way)
# ------------------------------------------------------------------------------------------------
class Native:
    """The raw ops, one stage at a time."""

    def __getattr__(self, name):
        return getattr(torch.ops.replicann, name)

    def layernorm_fwd_q8(self, x, r, w, b, eps):
        slot = torch.tensor([0.0, 3.0, 0.0, 0.0], device=x.device)  # a seeded delayed-scaling slot
        return torch.ops.replicann.layernorm_fwd_q8(x, r, w, b, eps, slot)[:4]

    def layernorm_bwd(self, dy, gh, h, w, mean, rstd, dw_accum=None, db_accum=None, dxs_accum=None):
        return torch.ops.replicann.layernorm_bwd(dy, gh, h, w, mean, rstd, dw_accum, db_accum, dxs_accum)


SLIPS = ("row_skipped", "mean_drops_column", "uncentred_variance", "partial_chunk_unwritten",
         "straddle_takes_padded_column", "onehot_off_by_one", "local_max_rescale_dropped", "partial_row_missing",
         "scratch_row_dirty")


def ln_bwd_blocks(M):
    """rn_ln_bwd_blocks: at most 2048 waves, four to a block, each block one partial row."""
    return (min(M, 2048) + 3) // 4


class Emu:
    """fp32 torch emulation of the ops (CPU tier).  ``slip``: one deliberate mistake (SLIPS), applied at
    ``slip_row`` where it concerns one row."""

    def __init__(self, slip=None, slip_row=2):
        assert slip is None or slip in SLIPS, slip
        self.slip, self.slip_row = slip, slip_row
        self.scratch = {}

    # ---- LayerNorm
    def layernorm_fwd(self, x, r, w, b, eps):
        M, E = x.shape
        h = x.float() if r is None else x.float() + r.float()
        hm = h
        if self.slip == "mean_drops_column":  # the last column never enters the row sum
            hm = h.clone()
            hm[:, E - 1] = 0
        mean = hm.sum(1) / E
        if self.slip == "uncentred_variance":  # E[h^2] - mean^2: cancels where the mean is far from 0
            var = (h * h).sum(1) / E - mean * mean
        else:
            var = ((h - mean[:, None])**2).sum(1) / E
        rstd = torch.rsqrt(var + eps)
        y = (h - mean[:, None]) * rstd[:, None] * w.float()
        if b is not None:
            y = y + b.float()
        y = y.to(torch.bfloat16)
        if self.slip == "row_skipped":  # the walk never reaches this row: its outputs are never written
            y[self.slip_row], mean[self.slip_row], rstd[self.slip_row] = 0, 0, 0
        return y, (x if r is None else h.to(torch.bfloat16)), mean, rstd

    def layernorm_fwd_q8(self, x, r, w, b, eps):
        return self.layernorm_fwd(x, r, w, b, eps)

    def layernorm_bwd(self, dy, gh, h, w, mean, rstd, dw_accum=None, db_accum=None, dxs_accum=None):
        M, E = dy.shape
        xh = (h.float() - mean[:, None]) * rstd[:, None]
        g = dy.float() * w.float()
        s1, s2 = g.sum(1) / E, (g * xh).sum(1) / E
        o = rstd[:, None] * (g - s1[:, None] - xh * s2[:, None])
        if gh is not None:
            o = o + gh.float()
        dx = o.to(torch.bfloat16)
        if self.slip == "partial_chunk_unwritten":  # the last 16-byte chunk of one row is not stored
            dx[self.slip_row, E - 8:] = 0
        rows = torch.ones(M, dtype=torch.bool)
        if self.slip == "partial_row_missing":  # block 1's partial row [dw | db | Σdx] never reaches the sums
            nw = 4 * ln_bwd_blocks(M)
            rows = (torch.arange(M) % nw) // 4 != 1
        rows = rows.to(dy.device)[:, None].float()
        dwp, dbp = (dy.float() * xh * rows).sum(0), (dy.float() * rows).sum(0)
        if dw_accum is not None and db_accum is not None:
            dw, db = dw_accum, db_accum
            dw.copy_((dwp + dw.float()).to(torch.bfloat16))
            db.copy_((dbp + db.float()).to(torch.bfloat16))
        else:
            dw, db = dwp.to(w.dtype), dbp.to(w.dtype)
        if dxs_accum is not None:
            dxs_accum.copy_(((dx.float() * rows).sum(0) + dxs_accum.float()).to(torch.bfloat16))
        return dx, dw, db

    # ---- softmax
    def softmax_fwd(self, x, scale):
        z = x.float() * scale
        e = torch.exp(z - z.amax(1, keepdim=True))
        return (e / e.sum(1, keepdim=True)).to(torch.bfloat16)

    def softmax_bwd(self, dy, y, scale):
        d = (dy.float() * y.float()).sum(1, keepdim=True)
        return (scale * y.float() * (dy.float() - d)).to(torch.bfloat16)

    # ---- cross-entropy
    def xent_fwd(self, logits, tgt, nvalid, ignore, write_grad=False):
        M, V = logits.shape
        if write_grad and V % 8 == 0 and V <= 65536:
            return self._xent_row2(logits, tgt, nvalid, ignore)
        nv = nvalid
        if self.slip == "straddle_takes_padded_column" and nvalid < V:
            nv = nvalid + 1
        z = logits[:, :nv].float()
        lse = torch.logsumexp(z, 1)
        ign = (tgt == ignore) | (tgt < 0) | (tgt >= nvalid)
        t = tgt.clamp(0, nvalid - 1)
        ar = torch.arange(M, device=logits.device)
        loss = torch.where(ign, torch.zeros_like(lse), lse - logits[ar, t].float())
        if write_grad:
            g = torch.zeros(M, V, device=logits.device)
            g[:, :nv] = torch.exp(z - lse[:, None])
            tt = self._onehot_at(t, nvalid)
            g[ar, tt] -= 1
            g[ign] = 0
            logits.copy_(g.to(torch.bfloat16))
        return loss, lse

    def _onehot_at(self, t, nvalid):
        if self.slip != "onehot_off_by_one":
            return t
        tt = t.clone()
        r = self.slip_row
        tt[r] = t[r] + 1 if int(t[r]) + 1 < nvalid else t[r] - 1
        return tt

    def _xent_row2(self, logits, tgt, nvalid, ignore):
        """xent_row2_k: 1024 threads, thread i owns the 8-column chunks i, i + 1024, ...; it keeps exp2 relative
        to its OWN maximum, as bf16, and rescales by 2^(m_own - lse) after the one block reduction."""
        M, V = logits.shape
        dev = logits.device
        CH = (V // 8 + 1023) // 1024
        P = CH * 1024 * 8
        nv = nvalid + 1 if self.slip == "straddle_takes_padded_column" and nvalid < V else nvalid
        x = torch.full((M, P), -INF, device=dev)
        x[:, :nv] = logits[:, :nv].float()
        xc = x.view(M, CH, 1024, 8)
        m_loc = xc.amax(dim=(1, 3))
        mL = torch.where(m_loc == -INF, torch.zeros_like(m_loc), m_loc * L2E)
        e32 = torch.exp2(xc * L2E - mL[:, None, :, None])
        s_loc = e32.sum(dim=(1, 3))
        e = e32.to(torch.bfloat16).float()
        Mx = m_loc.amax(1)
        S = (s_loc * torch.exp2((m_loc - Mx[:, None]) * L2E)).sum(1)
        lse = Mx + torch.log(S)
        f = torch.where(m_loc == -INF, torch.zeros_like(m_loc), torch.exp2(mL - lse[:, None] * L2E))
        if self.slip == "local_max_rescale_dropped":  # thread 1 of one row scales as if its maximum were the row's
            f[self.slip_row, 1] = torch.exp2((Mx[self.slip_row] - lse[self.slip_row]) * L2E)
        ign = (tgt == ignore) | (tgt < 0) | (tgt >= nvalid)
        t = tgt.clamp(0, nvalid - 1)
        ar = torch.arange(M, device=dev)
        xt = logits[ar, t].float()
        g = (e * f[:, None, :, None]).to(torch.bfloat16).view(M, P)[:, :V].clone()
        ft = f[ar, (t // 8) % 1024]
        et = torch.exp2(xt * L2E - mL[ar, (t // 8) % 1024]).to(torch.bfloat16).float()
        g[ar, self._onehot_at(t, nvalid)] = (et * ft - 1).to(torch.bfloat16)
        g[ign] = 0
        logits.copy_(g)
        return torch.where(ign, torch.zeros_like(lse), lse - xt), lse

    def xent_bwd(self, logits, tgt, lse, gscale, grad, nvalid, ignore):
        M, V = logits.shape
        p = torch.zeros(M, V, device=logits.device)
        p[:, :nvalid] = torch.exp(logits[:, :nvalid].float() - lse[:, None])
        ign = tgt == ignore
        ar = torch.arange(M, device=logits.device)
        p[ar, self._onehot_at(tgt.clamp(0, nvalid - 1), nvalid)] -= 1
        p = p * gscale
        p[ign] = 0
        grad.copy_(p.to(torch.bfloat16))

    # ---- embedding
    def embedding_fwd(self, ids, wte, wpe):
        T = ids.shape[-1] if ids.dim() >= 2 else ids.numel()
        x = wte[ids.reshape(-1)].float()
        if wpe is not None:
            x = x + wpe[torch.arange(ids.numel(), device=ids.device) % T].float()
        return x.to(torch.bfloat16).view(*ids.shape, wte.shape[1])

    def embedding_bwd(self, dx, ids, V, Tp):
        E = dx.shape[-1]
        T = ids.shape[-1] if ids.dim() >= 2 else ids.numel()
        d32 = torch.zeros(V, E, device=dx.device).index_add_(0, ids.reshape(-1), dx.float().reshape(-1, E))
        dwpe = torch.zeros(Tp, E, device=dx.device)
        if Tp:
            dwpe[:T] = dx.float().reshape(-1, T, E).sum(0)
        return d32.to(torch.bfloat16), dwpe.to(torch.bfloat16)

    def embedding_bwd_acc(self, dx, ids, gwte, gwpe):
        """The persistent scratch of the direct-accumulate path: all zero between calls."""
        V, E = gwte.shape
        T = ids.shape[-1] if ids.dim() >= 2 else ids.numel()
        d32 = self.scratch.setdefault((V, E), torch.zeros(V, E, device=dx.device))
        d32.index_add_(0, ids.reshape(-1), dx.float().reshape(-1, E))
        touched = ids.reshape(-1).unique()
        gwte[touched] = (gwte[touched].float() + d32[touched]).to(torch.bfloat16)
        keep = d32[touched[0]].clone()
        d32[touched] = 0
        if self.slip == "scratch_row_dirty":  # one touched row is not re-zeroed by the finish pass
            d32[touched[0]] = keep
        if gwpe is not None:
            gwpe[:T] = (gwpe[:T].float() + dx.float().reshape(-1, T, E).sum(0)).to(torch.bfloat16)


def backend(device):
    return Native() if torch.device(device).type == "cuda" else Emu()


def clear_caches():
    for f in (ln_inputs, ln_bwd_inputs, xent_inputs):
        f.cache_clear()


# ------------------------------------------------------------------------------------------------
# 1. LayerNorm forward
# ------------------------------------------------------------------------------------------------
def ln_nv(E):
    """The instantiation rn_ln_fwd / rn_ln_bwd pick: 16-byte chunks per lane, rounded up to {1, 2, 4, 8, 16}."""
    n = (E // 8 + 63) // 64
    return next(v for v in (1, 2, 4, 8, 16) if n <= v)


def _grid(shape, g, step=2.0**-8):
    """N(0, 1) rounded to multiples of 2^-8, as bf16: every sum of two is a multiple of 2^-8 below 32, exact in
    fp32, and needs up to 13 significand bits, so its rounding to bf16 is exercised."""
    return (torch.randn(shape, generator=g) / step).round().mul(step).to(torch.bfloat16)


# E at M = 9 (one row per wave, a ragged last block): NV 1 (8, 64, 96, 512), NV 2 with a nearly empty second
# chunk (520), 3 -> 4 (1032), 5 -> 8 (2056), NV 8 full (4096), NV 16 nearly empty (4104) and full (8192)
LN_FWD_E = [8, 64, 96, 512, 520, 1032, 2056, 4096, 4104, 8192]
# M at E = 64: fewer rows than a block, a ragged block, and (the forward grid is capped at 2048 blocks = 8192
# waves) 2 and 3 rows on some waves with a prefetch that must not run past M
LN_FWD_M = [1, 4, 5, 8197, 16389]
LN_FORMS = [(False, False), (False, True), (True, False), (True, True)]  # (residual, bias) / (gh, dxs)


@functools.lru_cache(maxsize=2)
def ln_inputs(device, M, E, residual, kind):
    g = gen(101 + 7 * M + E + (3 if residual else 0))
    if kind == "offset":  # rows of mean ~ 64 and spread ~ 1: an uncentred variance cancels
        x = (64 + torch.randn(M, E, generator=g)).to(torch.bfloat16)
    else:
        x = _grid((M, E), g) if residual else torch.randn(M, E, generator=g).to(torch.bfloat16)
    r = _grid((M, E), g) if residual else None
    w = (torch.rand(E, generator=g) + 0.5).to(torch.bfloat16)
    b = (0.5 * torch.randn(E, generator=g)).to(torch.bfloat16)
    mv = lambda t: None if t is None else t.to(device)
    return mv(x), mv(r), mv(w), mv(b)


def ln_stats_bounds(h64, E, eps=EPS):
    """(mu, rho, bound on the mean, bound on rstd) of float64 rows h.

    The kernel sums a row in fp32: each lane adds its 8·NV values in a chain, six shuffle levels add the 64
    lanes, one divide by E.  With d = 8·NV + 8 >= the depth of that tree plus the divide, the standard bound
    for a summation tree gives |mean - mu| <= d·u·mean_j|h_j| =: delta.
    The variance is the centred two-pass one, q = Σ (h_j - mean)² / E, about the COMPUTED mean; in exact
    arithmetic q = var + (mean - mu)², so the mean's error enters only in second order: relative (delta/sigma)²
    in q, with sigma = 1/rho = sqrt(var + eps).  The fp32 evaluation of q is another tree of depth d over
    non-negative terms, each with three roundings (subtract, square, add): relative (d + 3)·u; the eps add, the
    divide and rsqrtf (about 2 ulp) are inside the remaining 5·u.  rstd = (q + eps)^-1/2 halves a relative
    error; the bound keeps it whole: |rstd - rho| <= ((d + 8)·u + (delta/sigma)²)·rho."""
    d = 8 * ln_nv(E) + 8
    mu = h64.mean(1)
    var = ((h64 - mu[:, None])**2).mean(1)
    rho = 1 / torch.sqrt(var + eps)
    delta = d * U * h64.abs().mean(1)
    return mu, rho, delta, ((d + 8) * U + (delta * rho)**2) * rho


def case_ln_fwd(device, M, E, residual, bias, kind="plain", view=False, be=None):
    """layernorm_fwd, in two stages so that each bound is tight.

    Saved statistics (fp32) against float64: ln_stats_bounds.  One column left out of a row's mean at E = 8192
    moves it by |v|/E = 1.2e-4·|v|, about 15 times the bound.
    Outputs given the kernel's OWN saved statistics: with t = (h - mean)·rstd·w in float64,
    |y - (t + b)| <= 2^-8·|t + b| + 2^-20·(|t| + |b|): the one bf16 rounding, and 16·u for the four fp32
    operations (subtract, two multiplies, add: at most 4·u of |t| + |b|, and the rounding acts on the
    perturbed value).
    The residual form's h output is bitwise the one rounding of x + r: x and r are multiples of 2^-8 (``_grid``),
    so the fp32 add is exact, which is asserted on the reference.  In the plain form h is x itself.
    ``view``: x is rows 3 .. 3 + M of a larger sentinel-filled buffer; nothing in it may change.
    Branches: NV = ln_nv(E); M > 8192 puts more than one row on a wave (the grid-stride walk, the prefetch)."""
    be = be or backend(device)
    x, r, w, b = ln_inputs(str(device), M, E, residual, kind)
    b = b if bias else None
    big = None
    if view:
        big, x = sentinel_rows(x)
        x0 = x.clone()
    y, h, mean, rstd = be.layernorm_fwd(x, r, w, b, EPS)
    ck = Checks(f"ln_fwd M={M} E={E} NV={ln_nv(E)} res={int(residual)} bias={int(bias)} {kind}")
    h64 = x.double() if r is None else x.double() + r.double()
    if residual:
        assert bool(((x.float() + r.float()).double() == h64).all()), "precondition: the fp32 add x + r is exact"
        assert int((expect_bf16(h64).double() != h64).sum()) >= 0.1 * h64.numel(), "precondition: h rounds"
        ck.check("h", h, expect_bf16(h64))
    else:
        ck.check_true("h", h.data_ptr() == x.data_ptr(), "the plain form must return x itself as h")
    mu, rho, dmean, drstd = ln_stats_bounds(h64, E)
    ck.bound("mean", mean, mu, dmean)
    ck.bound("rstd", rstd, rho, drstd)
    t = (h64 - mean.double()[:, None]) * rstd.double()[:, None] * w.double()
    b64 = b.double().expand_as(t) if bias else torch.zeros_like(t)
    ck.bound("y given the saved statistics", y, t + b64, BF * (t + b64).abs() + 2.0**-20 * (t.abs() + b64.abs()))
    if view:
        ck.check_true("x view", rows_untouched(big, x0), "the buffer around (or under) the x view changed")
    LAST.clear()
    LAST["y"] = (y, (h64 - mu[:, None]) * rho[:, None] * w.double() + b64)
    ck.done()
    return y, h, mean, rstd


def case_ln_fwd_q8(device, M, E, residual, bias, be=None):
    """layernorm_fwd_q8's bf16 and fp32 outputs (y, h, mean, rstd) are bitwise layernorm_fwd's: the same
    kernel body, but its grid is capped at 4096 blocks, not 2048, so M = 16389 > 4·4096 still puts two rows on
    some waves.  (The e4m3 bytes: tests/test_fp8_ln_q8_gpu.py.)"""
    be = be or backend(device)
    x, r, w, b = ln_inputs(str(device), M, E, residual, "plain")
    b = b if bias else None
    ref = be.layernorm_fwd(x, r, w, b, EPS)
    got = be.layernorm_fwd_q8(x, r, w, b, EPS)
    ck = Checks(f"ln_fwd_q8 M={M} E={E} res={int(residual)} bias={int(bias)}")
    for name, a, e in zip(("y", "h", "mean", "rstd"), got, ref):
        ck.check(name, _as2d(a), _as2d(e))
    ck.done()


# ------------------------------------------------------------------------------------------------
# 2. LayerNorm backward
# ------------------------------------------------------------------------------------------------
LN_BWD_FORMS_E = [96, 520, 4104]  # all four (gh, dxs) forms at M = 2051: 3 waves walk two rows
LN_BWD_E = [8, 512, 1032, 2056, 4096, 8192]  # M = 9, plain: NV 1, 1, 4, 8, 8 and the full NV 16
LN_BWD_M = [1, 5, 2051, 4099]  # E = 64; the grid is capped at 2048 waves: 2 and 3 rows on some waves


@functools.lru_cache(maxsize=2)
def ln_bwd_inputs(device, M, E, lo=-8, hi=8, density=1.0):
    g = gen(211 + 5 * M + E)
    h = torch.randn(M, E, generator=g).to(torch.bfloat16)
    dy = int_operand((M, E), lo, hi, density=density, generator=g)
    gh = torch.randn(M, E, generator=g).to(torch.bfloat16)
    w = (torch.rand(E, generator=g) + 0.5).to(torch.bfloat16)
    return tuple(t.to(device) for t in (h, dy, gh, w))


def ln_bwd_depth(M):
    """D of the dw / Σdx bound: the rows one wave accumulates, the fold of a block's four waves, and the column
    kernel (rn_colsum1_k: at most 512 partial rows, so every wave chains ceil(B/16) of them and 16 wave sums
    fold).  Counted as the issue does, rows per wave + 4 + 16 + chain: a chain of n terms is n - 1 roundings
    (and the first add into 0 is exact), so the count has 4 to spare, which covers the 3 roundings inside one
    dy·x̂ term (subtract, multiply for x̂; the product)."""
    B = ln_bwd_blocks(M)
    return -(-M // (4 * B)) + 4 + 16 + -(-B // 16)


def case_ln_bwd(device, M, E, gh, dxs, accumulate=False, be=None, dy_range=(-8, 8)):
    """layernorm_bwd on h, mean, rstd of the forward (the emulation's or the kernel's own), dy integer-valued.

    dx, per element against float64 rstd·(g - s1 - x̂·s2) + gh with g = dy·w, x̂ = (h - mean)·rstd, s1 = mean(g),
    s2 = mean(g·x̂), all from the saved fp32 mean and rstd.  fp32 evaluation, d = 8·NV + 8 as in the forward:
      x̂ carries 2·u, g one; s1 is a tree of depth d over terms with 1·u: |Δs1| <= (d + 2)·u·mean|g|;
      s2 over terms with 4·u: |Δs2| <= (d + 6)·u·mean|g·x̂|;
      o = rstd·(g - s1 - x̂·s2): two subtractions, the product x̂·s2 (x̂'s 2·u, one more) and the multiply by rstd,
      at most 6·u of A = |g| + |s1| + |x̂·s2|, plus Δs1 and |x̂|·Δs2; the add of gh is 1·u of the result:
      fp = rstd·u·(6·A + (d + 2)·mean|g| + (d + 6)·|x̂|·mean|g·x̂|) + u·|dx|.
    The one bf16 rounding acts on the perturbed value: |dx - dx64| <= 2^-8·|dx64| + (1 + 2^-8)·fp.

    db, bitwise: dy in {-8 .. 8} and M <= 20000, so every ordering of every partial sum (the row walk, the
    four-wave LDS fold, the partial rows, the column kernel) is an integer below 2^24 and db is the one rounding
    of Σ_i dy.  A row dropped or counted twice anywhere changes the bits.
    ``accumulate``: dw_accum / db_accum hold integers and dy is sparse, so that |old + Σ| <= 256 is a bf16 value
    (asserted): db is then bitwise old + Σ; dw is held to its bound around old + dw64.
    dw, per column: 2^-8·|dw64| + D·u·Σ_i|dy·x̂| (ln_bwd_depth); dxs_accum (zeroed first) against the float64
    sum of the RETURNED bf16 dx, which is what the kernel sums: 2^-8·|s| + D·u·Σ_i|dx|.
    Branches: NV = ln_nv(E) (E = 8192: the full ln_bwd_k<16>, 96 KiB of LDS); M > 2048: more than one row per
    wave; the (GH, DXS) template forms; B = ln_bwd_blocks(M) partial rows into rn_colsum1_k."""
    be = be or backend(device)
    assert M <= 20000 and max(abs(v) for v in dy_range) <= 8
    h, dy, ghv, w = ln_bwd_inputs(str(device), M, E, dy_range[0], dy_range[1], 0.02 if accumulate else 1.0)
    ghv = ghv if gh else None
    _, _, mean, rstd = be.layernorm_fwd(h, None, w, None, EPS)
    g0 = gen(5 + M + E)
    dw0 = int_operand((E,), -64, 64, device=device, generator=g0) if accumulate else None
    db0 = int_operand((E,), -64, 64, device=device, generator=g0) if accumulate else None
    dw_acc, db_acc = (dw0.clone(), db0.clone()) if accumulate else (None, None)
    dxs_acc = torch.zeros(E, device=device, dtype=torch.bfloat16) if dxs else None
    dx, dw, db = be.layernorm_bwd(dy, ghv, h, w, mean, rstd, dw_acc, db_acc, dxs_acc)

    ck = Checks(f"ln_bwd M={M} E={E} NV={ln_nv(E)} gh={int(gh)} dxs={int(dxs)} acc={int(accumulate)}")
    d = 8 * ln_nv(E) + 8
    rs = rstd.double()[:, None]
    xh = (h.double() - mean.double()[:, None]) * rs
    g = dy.double() * w.double()
    s1, s2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    dx64 = rs * (g - s1 - xh * s2) + (ghv.double() if gh else 0)
    A = g.abs() + s1.abs() + (xh * s2).abs()
    fp = rs * U * (6 * A + (d + 2) * g.abs().mean(1, keepdim=True)
                   + (d + 6) * xh.abs() * (g * xh).abs().mean(1, keepdim=True)) + U * dx64.abs()
    ck.bound("dx", dx, dx64, BF * dx64.abs() + (1 + BF) * fp)

    sdy = dy.double().sum(0)
    assert float(dy.double().abs().sum(0).max()) + 64 < F32_EXACT_INT
    D = ln_bwd_depth(M)
    dw64, dwmag = (dy.double() * xh).sum(0), (dy.double() * xh).abs().sum(0)
    if accumulate:
        require_representable(db0.double() + sdy)
        assert bool((sdy != 0).any()), "precondition: the sparse dy still has non-zero column sums"
        ck.check("db accumulated", db.view(1, -1), expect_bf16(db0.double() + sdy).view(1, -1))
        ck.check_true("db accumulated", db.data_ptr() == db_acc.data_ptr(), "db is not the accumulate buffer")
        dw64, dwmag = dw64 + dw0.double(), dwmag + dw0.double().abs()
    else:
        ck.check("db", db.view(1, -1), expect_bf16(sdy).view(1, -1))
    ck.bound("dw", dw, dw64, BF * dw64.abs() + D * U * dwmag)
    if dxs:
        s64 = dx.double().sum(0)
        ck.bound("dxs", dxs_acc, s64, BF * s64.abs() + D * U * dx.double().abs().sum(0))
    LAST.clear()
    LAST.update(dx=(dx, dx64), dw=(dw, dw64), db=(db, sdy + (db0.double() if accumulate else 0)))
    ck.done()
    return dx, dw, db


# ------------------------------------------------------------------------------------------------
# 4. softmax and cross-entropy
# ------------------------------------------------------------------------------------------------
# V -> the kernels and branches it reaches (rn_xent_fwd: the register-row kernels take V % 8 == 0, V <= 65536)
XENT_V = {
    8: "xent_row2_k<1> / xent_row_k<1>, one chunk: 1023 threads without a column",
    1000: "CH 1 with 125 chunks: threads 125.. hold nothing (m = -inf, f = 0)",
    1024: "CH 1",
    8200: "CH 2, thread 0 alone owns a second chunk",
    16392: "CH 4 (3 chunks per thread rounded up)",
    57352: "CH 8",
    1002: "generic xent_fwd_k, scalar gradient; rows 16-byte aligned every fourth row only, so row_ms takes its "
          "vector loop on rows 0 and 4 and its scalar loop on the others",
    1003: "generic xent_fwd_k, scalar gradient branch; only row 0 aligned",
    65544: "generic xent_fwd_k above the register-row limit: vector row_ms and vector gradient",
}
XENT_M = 5
GSCALE = 0.375
FP_EXP = 2.0**-13  # above the relative fp32 error of a softmax probability while |logit| <= 100 (case_xent)


def xent_nvalids(V):
    return [8, 5, 1] if V == 8 else [V, V - 3, V - 47]


def minus_inf_run(n):
    """Columns [0, k) set to -inf: whole 8-column chunks, the first chunk of threads 0, 1, 2 (and in a scalar
    loop the first element of threads 0 .. 23).  None below 64 columns, where the run would be most of the row
    (at V = 8 all of it: a row with no finite logit has no softmax)."""
    return 24 if n >= 64 else 0


@functools.lru_cache(maxsize=2)
def xent_inputs(device, M, V, nvalid):
    """Base logits N(0, 3²) as bf16.  Row 1: a +60 spike.  Row 2: the chunks c with c % 256 in {1, 5} at -80:
    every column of the threads 1, 5 (mod 256) of the 1024-thread register-row kernels and of the 256-thread
    generic ones, so their local maxima are far below the row's.  Row 3: minus_inf_run.  Row 4: ignored.
    Targets: column 0 (row 0), n_valid - 1 (row 1), the first column of the chunk that holds n_valid - 1, which
    straddles n_valid when n_valid % 8 != 0 (row 2); later rows random."""
    assert M >= 5
    g = gen(307 + V + 3 * nvalid + M)
    x = 3 * torch.randn(M, V, generator=g)
    x[1, nvalid // 2] = 60
    chunk = torch.arange(V) // 8
    x[2, ((chunk % 256 == 1) | (chunk % 256 == 5))] = -80
    k = minus_inf_run(nvalid)
    x[3, :k] = -INF
    t = torch.randint(k, nvalid, (M,), generator=g) if nvalid > k else torch.zeros(M, dtype=torch.int64)
    t[0], t[1], t[2], t[4] = 0, nvalid - 1, (nvalid - 1) // 8 * 8, -100
    return x.to(torch.bfloat16).to(device), t.to(device)


def xent_ref(x, t, nvalid):
    """float64 (p - onehot, p, lse, per-row loss): the softmax over the valid columns; 0 in padded columns and
    in ignored rows."""
    M, V = x.shape
    z = x[:, :nvalid].double()
    lse = torch.logsumexp(z, 1)
    p = torch.zeros(M, V, dtype=torch.float64, device=x.device)
    p[:, :nvalid] = torch.exp(z - lse[:, None])
    ign = t < 0
    ar = torch.arange(M, device=x.device)
    tc = t.clamp(min=0)
    G = p.clone()
    G[ar, tc] -= 1
    G[ign], p[ign] = 0, 0
    loss = torch.where(ign, torch.zeros_like(lse), lse - x[ar, tc].double())
    return G, p, lse, loss


def case_xent(device, V, nvalid, mode, M=XENT_M, be=None):
    """Cross-entropy rows.  mode "fused": xent_fwd(write_grad=True) overwrites the logits with softmax - onehot
    (xent_row2_k, or the generic xent_fwd_k<true>).  mode "two_pass": xent_fwd(write_grad=False) (xent_row_k or
    xent_fwd_k<false>), then xent_bwd with gscale = 0.375 (xent_bwd_k).  XENT_V names the branch V reaches.

    Gradient, per element against float64 p - δ:
    |g - (p - δ)| <= (2^-7 + 2^-13)·p + 2^-8·|p - δ| + 2^-100 (times gscale in the two-pass form).
    xent_row2_k rounds e = exp2(x - m_own) to bf16 and the product e·f to bf16: two roundings of 2^-8 each,
    (1 + 2^-8)² - 1 = 2^-7 + 2^-16 of p.  The fp32 part (FP_EXP = 2^-13 of p, which also holds that 2^-16): the
    exp2 arguments x·log2e - m·log2e and m·log2e - lse·log2e carry u·(|x| + 2·|m| + |lse|)·log2e plus the error
    of lse (a sum tree, a log), v_exp_f32 about an ulp each: under u·(7·100 + 16) < 2^-14 while every finite logit
    is within ±100, which is asserted.  The target element adds the rounding of p - 1: 2^-8·|p - δ| (for the
    others it is the two-pass form's one rounding); 2^-100 covers flush to zero.  (The issue's form of this
    bound, 2^-7·p + 2^-8·|p - δ|, took a bf16 rounding for 2^-9; with the true 2^-8 the two roundings alone use
    up its 2^-7·p, so the fp32 term is added rather than folded in.)
    Exactly zero: the padded columns, the ignored row.  The targets at column 0, n_valid - 1 and in the chunk
    that straddles n_valid are also reported one by one.
    lse and the per-row loss: the tolerances of test_fused_lm_xent_rows_gpt2_vocab, 1e-3 and 2e-2, per row.
    The row with a -inf run has p = 0 there and a finite loss."""
    be = be or backend(device)
    x, t = xent_inputs(str(device), M, V, nvalid)
    G, p, lse64, loss64 = xent_ref(x, t, nvalid)
    assert bool(torch.isfinite(loss64).all()) and bool(torch.isfinite(G).all())
    ck = Checks(f"xent {mode} V={V} n_valid={nvalid} M={M}")
    scale = 1.0
    if mode == "fused":
        grad = x.clone()
        loss, lse = be.xent_fwd(grad, t, nvalid, -100, True)
    else:
        assert mode == "two_pass"
        logits = x.clone()
        loss, lse = be.xent_fwd(logits, t, nvalid, -100, False)
        ck.check("logits left alone", logits, x)
        grad = torch.full_like(x, SENTINEL)
        be.xent_bwd(logits, t, lse, torch.tensor([GSCALE], device=device), grad, nvalid, -100)
        scale = GSCALE
    assert float(x[torch.isfinite(x)].abs().max()) <= 100
    bound = scale * ((2.0**-7 + FP_EXP) * p + BF * G.abs()) + 2.0**-100
    ck.bound("gradient", grad, scale * G, bound)
    if nvalid < V:
        ck.zeros("padded columns", grad[:, nvalid:])
    ck.zeros("ignored row", grad[4:5])
    for r, name in ((0, "column 0"), (1, "n_valid - 1"), (2, "the chunk that straddles n_valid")):
        c = int(t[r])
        e = abs(float(grad[r, c]) - scale * float(G[r, c]))
        ck.check_true(f"target at {name}", e <= float(bound[r, c]),
                      f"row {r} column {c}: got {float(grad[r, c])!r}, float64 {scale * float(G[r, c])!r}")
    ck.bound("lse", lse, lse64, torch.full_like(lse64, 1e-3))
    ck.bound("loss", loss, loss64, torch.full_like(loss64, 2e-2))
    LAST.clear()
    LAST["grad"] = (grad[:, :nvalid], scale * G[:, :nvalid])
    ck.done()
    return grad


SOFTMAX_N = [1, 7, 8, 197, 256, 1000, 2049]  # 7 and 197: odd rows are not 16-byte aligned (the scalar loop)
SOFTMAX_M = 6


def case_softmax(device, N, scale, M=SOFTMAX_M, be=None):
    """softmax_fwd / softmax_bwd (one 256-thread block per row, row_ms then a scalar second pass).

    Forward, against float64 p = softmax(scale·x): |y - p| <= (2^-8 + 2^-13)·p + 2^-100: the one bf16 rounding,
    and FP_EXP for the fp32 evaluation (the argument x·scale - m carries u·(|z| + |z - m|), then the exp, the sum
    tree of depth ceil(N/2048) + 8 + 6 + 4, the reciprocal and the product: under u·350 < 2^-15 while |z| <= 100).
    (The issue wrote 2^-8·p taking the rounding for 2^-9; the rounding alone is 2^-8.)  Rows 0 (16-byte aligned: the vector loop) and 3 have a
    -inf run (minus_inf_run) where p = 0; row 1 has a spike.
    Backward on the STORED y, against float64 scale·y·(dy - d), d = Σ dy·y: d is a tree of depth
    D = ceil(N/256) + 6 + 4 (the thread's chain, the wave shuffles, the four waves) over products with 1·u:
    |Δd| <= (D + 1)·u·Σ|dy·y|; then one subtraction and two multiplies, at most 3·u of |dy| + |d|:
    fp = |scale·y|·((D + 1)·u·Σ|dy·y| + 3·u·(|dy| + |d|)), and |dx - dx64| <= 2^-8·|dx64| + (1 + 2^-8)·fp."""
    be = be or backend(device)
    g = gen(401 + N)
    x = 3 * torch.randn(M, N, generator=g)
    x[1, N // 2] = 30
    k = minus_inf_run(N)
    x[0, :k], x[3, :k] = -INF, -INF
    x = x.to(torch.bfloat16).to(device)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16).to(device)
    ck = Checks(f"softmax N={N} scale={scale}")
    y = be.softmax_fwd(x, scale)
    p = torch.softmax(x.double() * scale, 1)
    ck.bound("y", y, p, (BF + FP_EXP) * p + 2.0**-100)
    dx = be.softmax_bwd(dy, y, scale)
    y64, dy64 = y.double(), dy.double()
    d = (dy64 * y64).sum(1, keepdim=True)
    dx64 = scale * y64 * (dy64 - d)
    D = -(-N // 256) + 6 + 4
    fp = (scale * y64).abs() * ((D + 1) * U * (dy64 * y64).abs().sum(1, keepdim=True) + 3 * U * (dy64.abs() + d.abs()))
    if bool(torch.isfinite(y64).all()):
        ck.bound("dx on the stored y", dx, dx64, BF * dx64.abs() + (1 + BF) * fp)
    ck.done()
    return y


# ------------------------------------------------------------------------------------------------
# 5. embedding
# ------------------------------------------------------------------------------------------------
EMB_V, EMB_TP = 300, 48


def _table(shape, g):
    """N(0, 1) as bf16 with |v| >= 2^-9, so that the fp32 sum of two entries (< 2^4) is exact."""
    v = torch.randn(shape, generator=g)
    v = torch.where(v.abs() < 2.0**-9, torch.full_like(v, 2.0**-9), v)
    return v.to(torch.bfloat16)


def case_embedding_fwd(device, E, ids_shape, pos, be=None):
    """embedding_fwd: wte[id] + wpe[t] is one fp32 add and one rounding, so bitwise the rounding of the float64
    sum on ordinary random tables (the add's exactness is asserted).  ids 1-D and 2-D (t = position in the last
    dimension, T < wpe.size(0)), rows not a multiple of the 4 a block takes, ids 0 and V - 1 present."""
    be = be or backend(device)
    g = gen(503 + E + sum(ids_shape))
    V, T = EMB_V, ids_shape[-1]
    wte, wpe = _table((V, E), g).to(device), _table((T + 7, E), g).to(device)
    ids = torch.randint(0, V, ids_shape, generator=g)
    ids.view(-1)[0] = V - 1
    ids.view(-1)[-1] = 0 if ids.numel() > 1 else V - 1
    ids = ids.to(device)
    x = be.embedding_fwd(ids, wte, wpe if pos else None)
    ref = wte.double()[ids.reshape(-1)]
    if pos:
        pe = wpe.double()[torch.arange(ids.numel(), device=device) % T]
        assert bool(((wte.float()[ids.reshape(-1)] + pe.float()).double() == ref + pe).all()), \
            "precondition: the fp32 add is exact"
        ref = ref + pe
    ck = Checks(f"embedding_fwd E={E} ids={tuple(ids_shape)} pos={int(pos)}")
    ck.check_true("shape", tuple(x.shape) == tuple(ids_shape) + (E,), f"shape {tuple(x.shape)}")
    ck.check("x", x.reshape(-1, E), expect_bf16(ref))
    ck.done()


def emb_ids(g, B=3, T=41, V=EMB_V):
    """B·T = 123 positions: about a third on one hot id (~40 repeats), a few on V - 1 and 0, the rest uniform, so
    most of the V rows stay untouched."""
    ids = torch.randint(0, V, (B, T), generator=g)
    hot = int(torch.randint(1, V - 1, (1,), generator=g))
    ids[torch.rand(B, T, generator=g) < 0.33] = hot
    ids[0, 0], ids[B - 1, T - 1], ids[1, 3] = 0, V - 1, V - 1
    return ids


def case_embedding_bwd(device, E, be=None):
    """embedding_bwd with integer dx in {-4 .. 4}: every sum is an integer, so the fp32 atomics are exact in any
    order and dwte, dwpe are bitwise the float64 scatter: untouched rows zero, dwpe rows >= T (Tp > T) zero."""
    be = be or backend(device)
    g = gen(601 + E)
    ids = emb_ids(g).to(device)
    B, T = ids.shape
    dx = int_operand((B, T, E), -4, 4, device=device, generator=g)
    dwte, dwpe = be.embedding_bwd(dx, ids, EMB_V, EMB_TP)
    ref = torch.zeros(EMB_V, E, dtype=torch.float64, device=device).index_add_(0, ids.reshape(-1),
                                                                             dx.double().reshape(-1, E))
    refp = torch.zeros(EMB_TP, E, dtype=torch.float64, device=device)
    refp[:T] = dx.double().sum(0)
    require_representable(ref, refp)
    assert int(ids.unique().numel()) < EMB_V // 2 and int(ids.reshape(-1).bincount().max()) >= 30
    ck = Checks(f"embedding_bwd E={E}")
    ck.check("dwte", dwte, expect_bf16(ref))
    ck.check("dwpe", dwpe, expect_bf16(refp))
    ck.done()


def case_embedding_bwd_acc(device, E, calls=3, be=None, setenv=lambda k, v: None, deterministic=False):
    """embedding_bwd_acc (the direct-accumulate path: owner table and persistent scratch, which every call must
    leave zeroed and re-armed) into integer-valued prior gradients, ``calls`` times in a row on the same (V, E)
    with different id sets, each result asserted bitwise, untouched rows (the prior gradient) included.  A
    scratch row not re-zeroed or an owner not re-armed shows up in the second or third call.  Representable
    class: |prior + Σ| <= 256, asserted.  ``deterministic``: REPLICANN_DETERMINISTIC=1, the 2^40 fixed-point
    integer atomics (the binding reads it per call), also exact on integers."""
    be = be or backend(device)
    setenv("REPLICANN_DETERMINISTIC", "1" if deterministic else "0")
    g = gen(701 + E)
    gwte = int_operand((EMB_V, E), -64, 64, device=device, generator=g)
    gwpe = int_operand((EMB_TP, E), -64, 64, device=device, generator=g)
    ref, refp = gwte.double(), gwpe.double()
    ck = Checks(f"embedding_bwd_acc E={E} det={int(deterministic)}")
    for call in range(calls):
        ids = emb_ids(g).to(device)
        B, T = ids.shape
        dx = int_operand((B, T, E), -4, 4, density=0.5, device=device, generator=g)
        ref = ref.clone().index_add_(0, ids.reshape(-1), dx.double().reshape(-1, E))
        refp = refp.clone()
        refp[:T] += dx.double().sum(0)
        require_representable(ref, refp)
        be.embedding_bwd_acc(dx, ids, gwte, gwpe)
        ck.check(f"call {call + 1}: gwte", gwte, expect_bf16(ref))
        ck.check(f"call {call + 1}: gwpe", gwpe, expect_bf16(refp))
    LAST.clear()
    LAST["gwte"] = (gwte, ref)
    ck.done()
    return gwte


assert BF16_EXACT_INT == 256 and math.isclose(BF, 2.0**-8)
