"""The fp8 (OCP e4m3) KV cache's ops (csrc/kernels/attention_decode_kv8.hip).

Storage per layer: ``kv8`` uint8 (B, L, 2, H, D) e4m3fn bytes and ``kv_scale`` fp32 (B, L, 2, H), one scale
per (batch row, cache row, K|V, head), i.e. per D-element head vector — 68 bytes a head row at D = 64
instead of 128.  The scale rule is the quantisers' own (``ops.fp8.pow2_ceil``): scale = pow2_ceil(amax / 448)
with the quotient formed in fp32, 1 for an all-zero row, the smallest normal for a subnormal quotient; the
byte is e4m3(x · (1 / scale)), round to nearest even, saturating, subnormals and the sign of a zero kept, and
the value read back is decode(byte) · scale.  Every scale is a power of two, so x · (1 / scale) is exact and
each byte follows from the input alone: tests/test_kv_fp8*.py compare bytes and scales bitwise.  A row
carries its own scale, so an append needs no state, no calibration and nothing of a run's history.

``pos`` (1 or B int32 / int64 values on the inputs' device) is each batch row's write row, clamped to [0, L]
before use: no device value can index outside the buffers.  ``pos == L`` writes nothing, and neither does a
negative position (it reads as 0 cached rows).

On the GPU at head size 64 (``attention_decode_kv8``: L <= 1024) the ops are one launch each (inference only: an
input that requires grad, with grad enabled, raises).
Otherwise — CPU tensors, other head sizes, longer caches — the same semantics are composed from torch ops,
built on the float8 cast after the clamp; on the CPU that is the float reference (any float dtype in).
"""

from __future__ import annotations

import torch

from .. import _ext
from .attention import attention
from .fp8 import E4M3_MAX


def _quantize_rows(x):
    """(..., D) float -> (uint8 bytes (..., D), fp32 scales (...)) by the cache's rule."""
    f = x.float()
    amax = f.abs().amax(-1)
    # pow2_ceil on the bits of the fp32 quotient, as the kernel does (a quotient flushed to zero lands on the
    # smallest normal too)
    u = (amax / E4M3_MAX).view(torch.int32)
    e = u & 0x7F800000
    u = torch.where((u & 0x007FFFFF) != 0, e + 0x00800000, e)
    u = torch.where(u == 0, torch.full_like(u, 0x00800000), u)
    scale = torch.where(amax > 0, u.view(torch.float32), torch.ones_like(amax))
    q = (f * (1 / scale).unsqueeze(-1)).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def _decode(kv8, kv_scale):
    return kv8.view(torch.float8_e4m3fn).float() * kv_scale.unsqueeze(-1)


def kv8_dequantize(kv8, kv_scale):
    """The cache's values, decode(byte) · scale, as bf16 in ``kv8``'s shape.  Exact: an e4m3 value times a power
    of two is a bf16 value (down to bf16's smallest subnormal).  A composition of torch ops: the slow path and
    the tests use it."""
    return _decode(kv8, kv_scale).to(torch.bfloat16)


def _check(name, x, kv8, kv_scale, pos):
    B, H, D = x.shape[0], x.shape[3], x.shape[4]
    if kv8.dim() != 5 or kv8.dtype != torch.uint8 or (kv8.shape[0], *kv8.shape[2:]) != (B, 2, H, D):
        raise ValueError(f"{name}: kv8 must be uint8 (B, L, 2, H, D) for {tuple(x.shape)}, got {kv8.dtype} "
                         f"{tuple(kv8.shape)}")
    L = kv8.shape[1]
    if kv_scale.shape != (B, L, 2, H) or kv_scale.dtype != torch.float32:
        raise ValueError(f"{name}: kv_scale must be float32 {(B, L, 2, H)}, got {kv_scale.dtype} "
                         f"{tuple(kv_scale.shape)}")
    if pos.dim() != 1 or pos.shape[0] not in (1, B) or pos.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: pos must hold 1 or {B} int32 / int64 values, got {pos.dtype} {tuple(pos.shape)}")
    if not (kv8.device == kv_scale.device == pos.device == x.device):
        raise ValueError(f"{name}: every tensor must be on one device")
    return B, L, H, D


def _native(x, D):
    """The kernels take GPU bf16 inputs at head size 64.  The ops are inference only: an input that would record a
    graph is an error, not a reason to fall back."""
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError("the fp8 KV cache ops are inference only: call them under torch.no_grad() or on inputs that "
                           "do not require grad")
    return _ext.use_native(x) and D == 64 and x.dtype == torch.bfloat16


def _raw():
    """The kernels' ops (the tests wrap this to see that a call reached them)."""
    _ext.ops()  # the library is loaded
    return torch.ops.replicann_kv8


def _write_rows(new8, new_sc, kv8, kv_scale, p, writes):
    """Rows p[b] + i < L of new8 (B, T, 2, H, D) / new_sc (B, T, 2, H) into the cache for the batch rows that
    write (B,) — indexed writes on a clamped row index: a row that does not fit lands on L-1 carrying what L-1
    ends up holding anyway."""
    B, T = new8.shape[:2]
    L = kv8.shape[1]
    i = torch.arange(T, device=kv8.device).view(1, T)
    rows = (p.view(B, 1) + i).clamp(max=L - 1)  # (B, T) in range whatever pos holds
    src = rows - p.view(B, 1)  # <= i; a window row if >= 0 — the one that lands on L-1 —, else the buffer's own
    fits = (src >= 0) & (src < T) & writes.view(B, 1)
    at = rows.view(B, T, 1, 1, 1).expand_as(new8)
    pick = src.clamp(0, T - 1).view(B, T, 1, 1, 1).expand_as(new8)
    kv8.scatter_(1, at, torch.where(fits.view(B, T, 1, 1, 1), new8.gather(1, pick), kv8.gather(1, at)))
    at, pick = at[..., 0], pick[..., 0]
    kv_scale.scatter_(1, at, torch.where(fits.view(B, T, 1, 1), new_sc.gather(1, pick), kv_scale.gather(1, at)))


def kv8_append(kv_new, kv8, kv_scale, pos):
    """The prefill's append: ``kv_new`` (B, T, 2, H, D) — the key / value slice of the packed projection output —
    quantised row by row; rows ``pos[b] + i < L`` are written to ``kv8`` / ``kv_scale`` (in place), rows that do
    not fit are skipped and no other byte or scale changes."""
    if kv_new.dim() != 5 or kv_new.shape[2] != 2:
        raise ValueError(f"kv8_append: kv_new must be (B, T, 2, H, D), got {tuple(kv_new.shape)}")
    B, L, H, D = _check("kv8_append", kv_new, kv8, kv_scale, pos)
    if _native(kv_new, D):
        _raw().append(kv_new, kv8, kv_scale, pos.contiguous())
        return
    _write_rows(*_quantize_rows(kv_new), kv8, kv_scale, pos.long().clamp(0, L).expand(B), (pos >= 0).expand(B))


def attention_decode_kv8(qkv, kv8, kv_scale, pos, scale=None):
    """The one-token step's attention over an fp8 cache with the append folded in — ``qkv`` (B, 1, 3, H, D) the
    packed projection output -> (B, 1, H, D).  Inference only.

    Batch row b, head h: the new K and V vectors are quantised; if ``pos[b] < L`` their bytes and scales are
    written to row ``pos[b]`` (``pos[b] == L``: nothing is written).  The query attends cache rows
    0 .. pos[b]-1, dequantised, plus the new row with its quantised-then-dequantised value, which is not
    re-read from memory: a key has one value whenever it is read.  Rows at or past ``pos[b]`` are never
    loaded, bytes or scales, and may hold anything (the NaN byte 0x7F, NaN scales).  No atomics and a fixed
    reduction order: two runs agree bit for bit, and a 1-element ``pos`` gives the bits of B equal ones."""
    if qkv.dim() != 5 or qkv.shape[1] != 1 or qkv.shape[2] != 3:
        raise ValueError(f"attention_decode_kv8: qkv must be (B, 1, 3, H, D), got {tuple(qkv.shape)}")
    B, L, H, D = _check("attention_decode_kv8", qkv, kv8, kv_scale, pos)
    if scale is None:
        scale = D ** -0.5
    if _native(qkv, D) and L <= 1024:
        return _raw().attn_decode(qkv, kv8, kv_scale, pos.contiguous(), float(scale))
    dev = qkv.device
    p = pos.long().clamp(0, L).expand(B)
    new8, new_sc = _quantize_rows(qkv[:, :, 1:3])  # (B, 1, 2, H, D), (B, 1, 2, H)
    _write_rows(new8, new_sc, kv8, kv_scale, p, (pos >= 0).expand(B))
    # keys: cache rows < pos (the others zeroed: whatever they hold must not reach 0 · v), then the new row
    live = torch.arange(L, device=dev).view(1, L) < p.view(B, 1)
    kv = torch.cat([torch.where(live.view(B, L, 1, 1, 1), _decode(kv8, kv_scale), torch.zeros((), device=dev)),
                    _decode(new8, new_sc)], 1).to(qkv.dtype)
    open_ = torch.cat([live, torch.ones(B, 1, dtype=torch.bool, device=dev)], 1)
    bias = torch.zeros(B, 1, L + 1, device=dev).masked_fill_(~open_.view(B, 1, L + 1), float("-inf"))
    return attention(qkv[:, :, 0], kv[:, :, 0], kv[:, :, 1], scale=scale, bias=bias)
