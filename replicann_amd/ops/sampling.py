"""Token sampling from a row of logits: temperature, top-k, top-p (nucleus) and the draw.

GPU tensors go to the fused kernel (``csrc/kernels/sampling.hip``: one launch, graph-capturable);
CPU tensors to ``reference`` below, float64 ATen math of the SAME semantics — it is the oracle the
kernel is tested against.

Semantics (order-independent; selection works on the input logits, whose order a temperature > 0
preserves):

* ``temperature == 0``: the argmax, lowest index on ties; ``kept = 1``.  Else x_i = logit_i / temperature.
* top-k: keep i iff logit_i >= the k-th largest value — every tie at the k-th value stays
  (``decoding._sample`` drops ``logits < kth`` too).  ``top_k`` 0 / None / >= V: no filter.
* top-p, after top-k, with p = softmax of x over the top-k set: keep i iff the mass of the tokens with
  a STRICTLY GREATER logit is < top_p.  Without ties this is ``_sample``'s rule ("mass before a token
  already reaches top_p"); with ties — the normal case in bf16 — ``_sample`` cuts inside a tie group
  wherever ``torch.sort`` happened to put its members, this rule keeps the whole group.  The most
  likely token always stays.
* draw: e_i = exp(x_i - max) over the kept tokens, 0 elsewhere, Z = Σe: the smallest index i, in
  vocabulary order, with Σ_{j<=i} e_j > u·Z; if rounding leaves none, the last kept index of
  non-zero mass.  A -inf logit is never returned (it counts in ``kept`` when no filter removes it:
  ``kept`` is the size of the set that passed the filters).  NaN logits count as -inf.
"""

from __future__ import annotations

import torch

from .. import _ext

_M64 = (1 << 64) - 1


def hash_uniform(seed: int, idx: int) -> float:
    """``hash_uniform`` of ``csrc/include/common.h`` in Python integers: the uniform in [0, 1) that
    row ``idx`` draws from ``seed`` (a ``rng.next_seed`` value)."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (idx + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 40) / 16777216.0


def kept_mask(logits, temperature, top_k=None, top_p=None):
    """(keep (B, V) bool, e (B, V) float64): the tokens that pass the filters and their unnormalised
    masses exp((logit - max) / temperature), 0 outside the kept set.  ``temperature`` > 0."""
    x = logits.detach().double()
    x = torch.where(x.isnan(), torch.full_like(x, float("-inf")), x)
    B, V = x.shape
    m = x.max(-1, keepdim=True).values
    keep = torch.ones_like(x, dtype=torch.bool)
    if top_k and 0 < top_k < V:
        keep = x >= torch.topk(x, int(top_k), dim=-1).values[:, -1:]
    d = torch.where(x == m, torch.zeros_like(x), x - m)  # inf - inf: the maximum itself
    e = torch.where(keep, torch.exp(d / temperature), torch.zeros_like(x))
    if top_p is not None and top_p < 1.0:
        for b in range(B):  # per tie group: the mass of the strictly greater logits
            vals, inv = torch.unique(x[b], return_inverse=True)  # ascending
            mass = torch.zeros(vals.numel(), dtype=torch.float64).index_add_(0, inv, e[b])
            greater = mass.flip(0).cumsum(0).flip(0) - mass
            keep[b] &= (greater[inv] < top_p * e[b].sum()) | (x[b] == m[b])
        e = torch.where(keep, e, torch.zeros_like(e))
    return keep, e


def reference(logits, temperature, top_k, top_p, u):
    """The semantics above in float64 on the CPU: (tokens (B, 1) int64, kept (B,) int32)."""
    B, V = logits.shape
    if temperature == 0:
        x = logits.detach().double()
        x = torch.where(x.isnan(), torch.full_like(x, float("-inf")), x)
        return x.argmax(-1, keepdim=True), torch.ones(B, dtype=torch.int32)
    keep, e = kept_mask(logits, temperature, top_k, top_p)
    cdf = e.cumsum(-1)
    target = u.detach().double().reshape(B, 1) * e.sum(-1, keepdim=True)
    hit = cdf > target
    idx = torch.arange(V).expand(B, V)
    first = torch.where(hit, idx, torch.full_like(idx, V)).min(-1).values
    last = torch.where(e > 0, idx, torch.zeros_like(idx)).max(-1).values
    tokens = torch.where(first < V, first, last).unsqueeze(1)
    return tokens, keep.sum(-1).to(torch.int32)


def sample_logits(logits, temperature=1.0, top_k=None, top_p=None, *, u=None, seed_buf=None, params=None):
    """Sample one token per row of ``logits`` (B, V; bf16 or fp32, a column slice of a wider buffer is
    fine) → ``(tokens (B, 1) int64, kept (B,) int32)``, kept = the size of the set sampled from.

    ``temperature`` 0 = greedy; ``top_k`` (None / 0 = off) and ``top_p`` (None / 1 = off) as in the
    module docstring.  ``params``: a 3-element fp32 tensor (temperature, top_k, top_p) on the logits'
    device that overrides the three (0 / 1 = off) — a captured graph reads the settings from it.
    Randomness: exactly one of ``u`` ((B,) fp32 uniforms in [0, 1)) and, on the GPU, ``seed_buf`` (a
    1-element int64 tensor from ``ops.rng.next_seed``: row b draws ``hash_uniform(seed, b)``)."""
    if logits.dim() != 2:
        raise ValueError(f"sample_logits: logits must be (B, V), got {tuple(logits.shape)}")
    if (u is None) == (seed_buf is None):
        raise ValueError("sample_logits: exactly one of u and seed_buf must be given")
    top_k = 0 if top_k is None else int(top_k)
    top_p = 1.0 if top_p is None else float(top_p)
    if params is None and not (temperature >= 0 and top_k >= 0 and 0.0 < top_p <= 1.0):
        raise ValueError(f"sample_logits: need temperature >= 0, top_k >= 0 and top_p in (0, 1], got "
                         f"{temperature}, {top_k}, {top_p}")
    if logits.is_cuda:
        if not _ext.available():
            raise RuntimeError(f"sample_logits: native extension not loaded: {_ext.load_error()}")
        if params is not None:  # the host values are unused: pass valid ones
            temperature, top_k, top_p = 1.0, 0, 1.0
        return _ext.ops().sample_logits(logits.detach(), float(temperature), top_k, top_p, u, seed_buf, params)
    if seed_buf is not None:
        raise ValueError("sample_logits: seed_buf is a device seed; CPU logits take explicit uniforms u")
    if params is not None:
        temperature, k, top_p = (float(v) for v in params.tolist())
        top_k = int(k) if k >= 1 else 0
    return reference(logits, float(temperature), top_k, top_p, u)
