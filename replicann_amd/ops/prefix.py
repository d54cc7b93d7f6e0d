"""The one-token attention of n samples per prompt over one shared prompt cache
(csrc/kernels/attention_decode_prefix.hip).

Storage per layer: ``prefix_kv`` (G, P, 2, H, D), the G prompts' keys / values, written by the prefill and read only
from then on, and ``kv`` (B, L, 2, H, D) with B = G · n, each sample's own tail: the keys / values of the tokens it
has generated.  Batch row b is sample b % n of prompt g = b // n.  ``prefix_len`` (G,) and ``pos`` (B,) are int32 /
int64 on the inputs' device, clamped to [0, P] and [0, L] before use: no device value can index outside a buffer.

On the GPU — bf16, head size 64, P <= 1024, L <= 1024, n <= 64, rows that can move as 16-byte vectors — the op is
two launches (inference only: an input that requires grad, with grad enabled, raises).  Otherwise — CPU tensors,
other head sizes, more samples — the same semantics are composed from torch ops; on the CPU that is the float
reference (any float dtype in).
"""

from __future__ import annotations

import torch

from .. import _ext
from .attention import attention

# the kernels for the shapes they take (a bench / test hook, not an env knob: False runs the composed path on the
# GPU too — scripts/decode_bench.py --samples times the kernels against it)
PREFIX_NATIVE = True


def _raw():
    """The kernels' ops (the tests wrap this to see that a call reached them)."""
    _ext.ops()  # the library is loaded
    return torch.ops.replicann_prefix


def _rows16(t):
    """Can the kernels move ``t``'s head rows as 16-byte vectors?"""
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % 8 == 0 and s >= 0 for s in t.stride()[:-1])


def _dense(kv):
    """A (B, L, 2, H, D) layout whose rows do not overlap: the append writes through the strides."""
    B, L, _, H, D = kv.shape
    sb, st, s2, sh, _ = kv.stride()
    return sh >= D and s2 >= H * sh and st >= 2 * s2 and (B == 1 or sb >= L * st)


def takes_native(qkv, prefix_kv, kv):
    """Do the kernels take this call?  (The arguments have passed ``attention_decode_prefix``'s checks.)"""
    n = qkv.shape[0] // prefix_kv.shape[0]
    return (PREFIX_NATIVE and _ext.use_native(qkv) and qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 64
            and prefix_kv.shape[1] <= 1024 and kv.shape[1] <= 1024 and n <= 64
            and _rows16(qkv) and _rows16(prefix_kv) and _rows16(kv) and _dense(kv))


def attention_decode_prefix(qkv, prefix_kv, prefix_len, kv, pos, scale=None):
    """The one-token step's attention for n samples per prompt, the append folded in — ``qkv`` (B, 1, 3, H, D) the
    packed projection output, B = G · n -> (B, 1, H, D).  Inference only.

    Row b of prompt g = b // n: the new K and V vectors are copied bit for bit to ``kv[b, pos[b]]`` if
    ``pos[b] < L`` (otherwise nothing is written; no other element of ``kv`` and none of ``prefix_kv`` changes).
    The query attends prefix rows < ``prefix_len[g]``, tail rows < ``pos[b]`` and its own new row, which is taken
    from ``qkv`` and not re-read from memory.  Prefix rows at or past prefix_len[g] and tail rows at or past pos[b]
    are never loaded and may hold anything (NaN bit patterns).  No atomics and a fixed reduction order: two runs
    agree bit for bit.

    The kernels read each prompt's rows once per (prompt, head, key split) — the samples are the MFMA's column
    dimension — and write fp32 partials that a second launch merges with the row's tail and new row.  The composed
    path zeroes the rows that must not be read in a scratch copy and masks them with a -inf bias."""
    if qkv.dim() != 5 or qkv.shape[1] != 1 or qkv.shape[2] != 3:
        raise ValueError(f"attention_decode_prefix: qkv must be (B, 1, 3, H, D), got {tuple(qkv.shape)}")
    B, H, D = qkv.shape[0], qkv.shape[3], qkv.shape[4]
    if prefix_kv.dim() != 5 or tuple(prefix_kv.shape[2:]) != (2, H, D) or prefix_kv.shape[0] < 1 or prefix_kv.shape[1] < 1:
        raise ValueError(f"attention_decode_prefix: prefix_kv must be (G, P, 2, H, D) for qkv {tuple(qkv.shape)}, got "
                         f"{tuple(prefix_kv.shape)}")
    G, P = prefix_kv.shape[:2]
    if B < 1 or B % G != 0:
        raise ValueError(f"attention_decode_prefix: the batch {B} is not a multiple of the {G} prompts")
    n = B // G
    if kv.dim() != 5 or (kv.shape[0], *kv.shape[2:]) != (B, 2, H, D) or kv.shape[1] < 1:
        raise ValueError(f"attention_decode_prefix: kv must be (B, L, 2, H, D) for qkv {tuple(qkv.shape)}, got "
                         f"{tuple(kv.shape)}")
    L = kv.shape[1]
    for name, t, count in (("prefix_len", prefix_len, G), ("pos", pos, B)):
        if t.shape != (count,) or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"attention_decode_prefix: {name} must be ({count},) int32 / int64, got {t.dtype} "
                             f"{tuple(t.shape)}")
    if not (prefix_kv.device == kv.device == prefix_len.device == pos.device == qkv.device):
        raise ValueError("attention_decode_prefix: every tensor must be on one device")
    if not (prefix_kv.dtype == kv.dtype == qkv.dtype):
        raise ValueError(f"attention_decode_prefix: qkv, prefix_kv and kv must share a dtype, got {qkv.dtype}, "
                         f"{prefix_kv.dtype}, {kv.dtype}")
    if torch.is_grad_enabled() and (qkv.requires_grad or prefix_kv.requires_grad or kv.requires_grad):
        raise RuntimeError("attention_decode_prefix is inference only: call it under torch.no_grad() or on inputs "
                           "that do not require grad")
    if scale is None:
        scale = D ** -0.5
    if takes_native(qkv, prefix_kv, kv):
        return _raw().attn_decode(qkv, prefix_kv, prefix_len.contiguous(), kv, pos.contiguous(), float(scale))
    dev = qkv.device
    p = pos.long().clamp(0, L)
    plen = prefix_len.long().clamp(0, P).repeat_interleave(n)  # (B,)
    # the append, on a clamped row index: a row that does not fit lands on L-1 carrying what L-1 holds anyway
    at = p.clamp(max=L - 1).view(B, 1, 1, 1, 1).expand(B, 1, 2, H, D)
    kv.scatter_(1, at, torch.where((p < L).view(B, 1, 1, 1, 1), qkv[:, :, 1:3], kv.gather(1, at)))
    # keys: prefix rows < prefix_len, tail rows < pos (the others zeroed: whatever they hold must not reach 0 · v),
    # then the new row
    zero = torch.zeros((), dtype=kv.dtype, device=dev)
    live_p = torch.arange(P, device=dev).view(1, P) < plen.view(B, 1)
    live_t = torch.arange(L, device=dev).view(1, L) < p.view(B, 1)
    pre = torch.where(live_p.view(B, P, 1, 1, 1), prefix_kv.repeat_interleave(n, 0), zero)
    tail = torch.where(live_t.view(B, L, 1, 1, 1), kv, zero)
    keys = torch.cat([pre, tail, qkv[:, :, 1:3]], 1)
    open_ = torch.cat([live_p, live_t, torch.ones(B, 1, dtype=torch.bool, device=dev)], 1)
    bias = torch.zeros(B, 1, P + L + 1, device=dev).masked_fill_(~open_.view(B, 1, P + L + 1), float("-inf"))
    return attention(qkv[:, :, 0], keys[:, :, 0], keys[:, :, 1], scale=scale, bias=bias)
