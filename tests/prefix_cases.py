"""Cases of the shared-prompt one-token attention (replicann_amd.ops.prefix,
csrc/kernels/attention_decode_prefix.hip), shared by the CPU tier (tests/test_shared_prefix.py) and the GPU tier
(tests/test_shared_prefix_gpu.py).  A plain module, not a conftest.

The reference is ``ops.attention_reference`` in fp32, row by row, over
``cat(prefix[g, :plen], tail[b, :pos], new row)`` of the buffers as they were before the call.  Buffers are filled
with a NaN bit pattern past the lengths: a row the op must not read makes the output non-finite, and the bitwise
comparison after the call is over integer views, so NaN payloads count.
"""

import torch

NAN16 = 0x7FC5  # a bf16 NaN with a payload
NAN32 = 0x7FC00A5A  # an fp32 one


def nan_fill(t):
    """Every element of ``t`` (bf16 / fp32) set to the NaN pattern of its width."""
    if t.element_size() == 2:
        t.view(torch.int16).fill_(NAN16)
    else:
        t.view(torch.int32).fill_(NAN32)
    return t


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def clamp(v, hi):
    return [min(max(int(x), 0), hi) for x in v]


def make(G, n, H, D, P, L, plen, pos, dtype, device, seed=0):
    """(qkv (B, 1, 3, H, D), prefix_kv (G, P, 2, H, D), kv (B, L, 2, H, D)): random rows below the (clamped) lengths
    ``plen`` (G host integers) and ``pos`` (B), the NaN pattern at and past them."""
    B = G * n
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, 1, 3, H, D, generator=gen).to(dtype)
    prefix = nan_fill(torch.empty(G, P, 2, H, D, dtype=dtype))
    kv = nan_fill(torch.empty(B, L, 2, H, D, dtype=dtype))
    for g, k in enumerate(clamp(plen, P)):
        prefix[g, :k] = torch.randn(k, 2, H, D, generator=gen).to(dtype)
    for b, k in enumerate(clamp(pos, L)):
        kv[b, :k] = torch.randn(k, 2, H, D, generator=gen).to(dtype)
    return qkv.to(device), prefix.to(device), kv.to(device)


def reference(qkv, prefix, kv, plen, pos, scale=None):
    """fp32 (B, 1, H, D) on the CPU from the buffers BEFORE the call."""
    from replicann_amd.ops import attention_reference
    qkv, prefix, kv = qkv.float().cpu(), prefix.float().cpu(), kv.float().cpu()
    B, G, D = qkv.shape[0], prefix.shape[0], qkv.shape[-1]
    n = B // G
    plen, pos = clamp(plen, prefix.shape[1]), clamp(pos, kv.shape[1])
    out = []
    for b in range(B):
        rows = torch.cat([prefix[b // n, :plen[b // n]], kv[b, :pos[b]], qkv[b, :, 1:3]], 0).unsqueeze(0)
        out.append(attention_reference(qkv[b:b + 1, :, 0], rows[:, :, 0], rows[:, :, 1], scale or D ** -0.5))
    return torch.cat(out, 0)


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def assert_buffers(what, qkv, prefix, kv, before, pos):
    """After the call: row pos[b] of ``kv`` holds the new K / V bitwise (if it fits), every other element of ``kv``
    and all of ``prefix`` is what ``before`` = (prefix, kv) held — compared as integer views."""
    want = before[1].clone()
    L = want.shape[1]
    for b, p in enumerate(clamp(pos, L)):
        if p < L:
            want[b, p] = qkv[b, 0, 1:3]
    assert torch.equal(bits(prefix), bits(before[0])), f"{what}: the prefix changed"
    same = bits(kv) == bits(want)
    assert bool(same.all()), f"{what}: {int((~same).sum())} tail elements differ from the expected buffer"


def run_case(op, G, n, H, D, P, L, plen, pos, dtype, device, index_dtype=torch.int64, seed=0):
    """One call on NaN-padded buffers: finite, the buffers right afterwards.  Returns (output, reference, inputs)."""
    qkv, prefix, kv = make(G, n, H, D, P, L, plen, pos, dtype, device, seed)
    before = (prefix.clone(), kv.clone())
    ref = reference(qkv, prefix, kv, plen, pos)
    out = op(qkv, prefix, torch.tensor(plen, dtype=index_dtype, device=device), kv,
             torch.tensor(pos, dtype=index_dtype, device=device))
    assert out.shape == (G * n, 1, H, D) and out.dtype == dtype
    assert bool(torch.isfinite(out).all()), "a row at or past a length was read"
    assert_buffers(f"G={G} n={n} plen={plen} pos={pos}", qkv, prefix, kv, before, pos)
    return out, ref, (qkv, before)
