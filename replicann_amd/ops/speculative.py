"""Speculative sampling: verification of K draft tokens per row against the target's distributions.

GPU tensors go to the fused kernel (``csrc/kernels/spec_verify.hip``: one workgroup per (row, window
position) and a one-thread-per-row combine, graph-capturable); CPU tensors to ``reference`` below,
float64 ATen math of the SAME semantics, built on ``sampling.kept_mask`` so that the filters cannot
diverge from ``sample_logits`` — it is the oracle the kernel is tested against.

Semantics (Leviathan et al. 2023; Chen et al. 2023), per batch row, window positions i = 0 .. K:

* p_i: the distribution ``sample_logits`` draws from on ``target_logits[b, i]`` — the kept set of the
  top-k / top-p filters and its masses exp((logit - max) / temperature), normalised; q_i (i < K): the
  same on ``draft_logits[b, i]``, the row the draft token d_i = ``drafts[b, i]`` was drawn from.
* acceptance: d_i is accepted iff ``u_acc · q_i(d_i) < p_i(d_i)``; a token with q_i(d_i) = 0 (one the
  draft's own filter would not emit) is rejected.  ``matched`` = a, the number of LEADING accepted
  drafts: what follows the first rejection does not count.
* the extra token: for a < K a draw from the residual max(p_a - q_a, 0) — or from p_a where the
  residual has no mass (p_a = q_a on the kept set) — and for a = K the bonus token, a draw from p_K.
  Every draw is ``sample_logits``'s: the smallest index, in vocabulary order, whose cumulative weight
  exceeds ``u_draw`` · (the total weight); if rounding leaves none, the last index of non-zero weight.
* ``tokens[b]`` = d_1 .. d_a, the extra token, then zeros.
* ``temperature == 0``: p is one-hot at the target's argmax (lowest index on ties, NaN = -inf).  A
  draft is accepted iff it IS that argmax and the extra token is the argmax of position a: exactly
  ``decoding.accept`` on the arg-maxes.  The draft logits are not read (with d_i the draft's own
  argmax this is the rule above for one-hot p and q).
* randomness: position (b, i) uses two uniforms in [0, 1): ``u[b, i, 0]`` decides the acceptance,
  ``u[b, i, 1]`` draws the resample / bonus token; from a device seed they are
  ``hash_uniform(seed, 2·(b·(K+1)+i))`` and the same ``+ 1``.
"""

from __future__ import annotations

import torch

from .. import _ext
from .sampling import kept_mask


def _draw(w, u):
    """Inverse CDF in index order over the weights ``w`` (N, V) float64 at ``u`` (N,): ``sample_logits``'s rule."""
    N, V = w.shape
    hit = w.cumsum(-1) > (u.double() * w.sum(-1)).unsqueeze(1)
    idx = torch.arange(V).expand(N, V)
    first = torch.where(hit, idx, torch.full_like(idx, V)).min(-1).values
    last = torch.where(w > 0, idx, torch.zeros_like(idx)).max(-1).values
    return torch.where(first < V, first, last)


def _probs(logits, temperature, top_k, top_p):
    e = kept_mask(logits.reshape(-1, logits.shape[-1]), temperature, top_k, top_p)[1]
    return (e / e.sum(-1, keepdim=True)).view(logits.shape)


def reference(target_logits, draft_logits, drafts, temperature, top_k, top_p, u):
    """The semantics above in float64 on the CPU: (tokens (B, K+1) int64, matched (B,) int64)."""
    B, K = drafts.shape
    j = torch.arange(K + 1).view(1, K + 1)
    if temperature == 0:
        x = target_logits.detach().double()
        cand = torch.where(x.isnan(), torch.full_like(x, float("-inf")), x).argmax(-1)
        ok = drafts == cand[:, :K]
    else:
        p = _probs(target_logits, temperature, top_k, top_p)  # (B, K+1, V)
        q = _probs(draft_logits, temperature, top_k, top_p)  # (B, K, V)
        at = drafts.unsqueeze(-1)
        pd, qd = p[:, :K].gather(2, at).squeeze(2), q.gather(2, at).squeeze(2)
        ok = (qd > 0) & (u[..., 0].double().clamp(0, 1)[:, :K] * qd < pd)
        res = (p[:, :K] - q).clamp(min=0)
        res = torch.where(res.sum(-1, keepdim=True) > 0, res, p[:, :K])  # no residual mass: from p
        w = torch.cat([res, p[:, K:]], 1)  # position K draws the bonus token from p_K
        cand = _draw(w.view(B * (K + 1), -1), u[..., 1].reshape(-1)).view(B, K + 1)
    matched = ok.long().cumprod(1).sum(1)
    a = matched.view(B, 1)
    padded = torch.cat([drafts, torch.zeros(B, 1, dtype=drafts.dtype)], 1)
    tokens = torch.where(j < a, padded, torch.where(j == a, cand, torch.zeros_like(cand)))
    return tokens, matched


def speculative_verify(target_logits, draft_logits, drafts, temperature, top_k=None, top_p=None, *, u=None,
                       seed_buf=None, params=None, check_drafts=True):
    """Verify K draft tokens per row: ``target_logits`` (B, K+1, V) — the target's logits after the
    pending token and after each draft —, ``draft_logits`` (B, K, V) — the rows the drafts were drawn
    from — and ``drafts`` (B, K) int64 → ``(tokens (B, K+1) int64, matched (B,) int64)``: the accepted
    drafts followed by one resampled / bonus token and zeros, and the number of accepted drafts.

    Logits are bf16 or fp32 (both the same), with a unit last stride and row strides >= V; 1 <= K <= 15.
    ``temperature`` / ``top_k`` / ``top_p`` / ``params`` as in ``sample_logits``.  Randomness: exactly
    one of ``u`` ((B, K+1, 2) fp32 uniforms: acceptance draw, resample / bonus draw) and, on the GPU,
    ``seed_buf`` (a 1-element int64 tensor from ``ops.rng.next_seed``).  ``check_drafts``: raise for a
    draft outside [0, V) — on the GPU that reads the drafts' range on the host (a sync; not possible
    inside a graph capture); without it the kernel rejects such a draft and never returns it."""
    if target_logits.dim() != 3 or draft_logits.dim() != 3 or drafts.dim() != 2:
        raise ValueError(f"speculative_verify: need target (B, K+1, V), draft (B, K, V) and drafts (B, K), got "
                         f"{tuple(target_logits.shape)}, {tuple(draft_logits.shape)}, {tuple(drafts.shape)}")
    B, K1, V = target_logits.shape
    K = K1 - 1
    if not 1 <= K <= 15:
        raise ValueError(f"speculative_verify: K must be in 1..15, got {K}")
    if tuple(draft_logits.shape) != (B, K, V) or tuple(drafts.shape) != (B, K):
        raise ValueError(f"speculative_verify: need target (B, K+1, V), draft (B, K, V) and drafts (B, K), got "
                         f"{tuple(target_logits.shape)}, {tuple(draft_logits.shape)}, {tuple(drafts.shape)}")
    if target_logits.dtype != draft_logits.dtype:
        raise ValueError(f"speculative_verify: target and draft logits differ in dtype: {target_logits.dtype}, "
                         f"{draft_logits.dtype}")
    if drafts.dtype != torch.long:
        raise ValueError(f"speculative_verify: drafts must be int64, got {drafts.dtype}")
    if (u is None) == (seed_buf is None):
        raise ValueError("speculative_verify: exactly one of u and seed_buf must be given")
    top_k = 0 if top_k is None else int(top_k)
    top_p = 1.0 if top_p is None else float(top_p)
    if params is None and not (temperature >= 0 and top_k >= 0 and 0.0 < top_p <= 1.0):
        raise ValueError(f"speculative_verify: need temperature >= 0, top_k >= 0 and top_p in (0, 1], got "
                         f"{temperature}, {top_k}, {top_p}")
    if target_logits.is_cuda:
        if not _ext.available():
            raise RuntimeError(f"speculative_verify: native extension not loaded: {_ext.load_error()}")
        _ext.ops()
        if params is not None:  # the host values are unused: pass valid ones
            temperature, top_k, top_p = 1.0, 0, 1.0
        return torch.ops.replicann_spec.verify(target_logits.detach(), draft_logits.detach(), drafts,
                                               float(temperature), top_k, top_p, u, seed_buf, params,
                                               bool(check_drafts))
    if draft_logits.is_cuda or drafts.is_cuda:
        raise ValueError("speculative_verify: target_logits, draft_logits and drafts must be on one device")
    if seed_buf is not None:
        raise ValueError("speculative_verify: seed_buf is a device seed; CPU logits take explicit uniforms u")
    if tuple(u.shape) != (B, K + 1, 2):
        raise ValueError(f"speculative_verify: u must be (B, K+1, 2) = {(B, K + 1, 2)}, got {tuple(u.shape)}")
    if check_drafts and B and not (0 <= int(drafts.min()) and int(drafts.max()) < V):
        raise ValueError(f"speculative_verify: drafts must lie in [0, {V})")
    if params is not None:
        temperature, k, top_p = (float(v) for v in params.tolist())
        top_k = int(k) if k >= 1 else 0
    return reference(target_logits, draft_logits, drafts, float(temperature), top_k, top_p, u)
