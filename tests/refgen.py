"""Deterministic weights / inputs shared by scripts/gen_reference_fixtures.py (which runs the
reference's own code on the CPU, fp32) and tests/test_reference_parity_gpu.py (which runs the native
bf16 GPU path on a GPU box, where there is no copy of the reference), and the sharded store of the
recorded results under tests/golden/."""

import glob
import os

import torch

CASES = [  # name, block, n_heads, E, T, extra ctor kwargs
    ("enc_h12_e768", "TransformerEncoder", 12, 768, 128, {}),
    ("enc_h8_e256", "TransformerEncoder", 8, 256, 96, {}),
    ("enc_h4_e512", "TransformerEncoder", 4, 512, 64, {}),
    ("dec_h12_e768", "TransformerDecoder", 12, 768, 128, {"context_size": 256}),
    ("dec_h8_e256", "TransformerDecoder", 8, 256, 80, {"context_size": 256}),
]
CROSS = ("xdec_h12_e768", 12, 768, 96, 64)  # name, H, E, T_src, T_tgt


def det_state_dict(module, seed):
    """Weights drawn from a seeded generator in state_dict key order (independent of either
    implementation's init); LayerNorms near identity, buffers (the decoder mask) kept."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in module.state_dict().items():
        if k.endswith("_attn_mask"):
            sd[k] = v.clone()
        elif k.endswith("ln.weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(v.shape, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(v.shape, generator=g)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * (v.shape[-1] ** -0.5)
    return sd


def det_input(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * 0.5


def det_grad(shape, seed):
    g = torch.Generator().manual_seed(seed + 7)
    return torch.randn(shape, generator=g)


# Parameter-gradient parity: train mode, every dropout p = 0 (the reference's
# head dropout is fixed at 0.1 by its constructor — quirk Q4 — so it is zeroed on the module), the
# reference's per-parameter .grad recorded for every state_dict key; small widths keep the fixture
# small (head sizes 64 and 32 both covered).
GRAD_CASES = [  # name, block, n_heads, E, T, extra ctor kwargs
    ("genc_h4_e256", "TransformerEncoder", 4, 256, 64, {}),
    ("genc_h8_e256", "TransformerEncoder", 8, 256, 72, {}),
    ("gdec_h4_e256", "TransformerDecoder", 4, 256, 80, {"context_size": 128}),
]
GRAD_CROSS = ("gxdec_h4_e256", 4, 256, 64, 48)  # encoder (return_kv) -> cross decoder, both trained


# The recorded reference results are kept as shards under tests/golden/<stem>.NN.pt, each well under
# 1 MiB: a nested dict of tensors is flattened to "case/sub/key" paths, packed greedily, and put
# together again on load (weights_only: tensors, strings, numbers, lists).
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHARD_BYTES = 768 * 1024


def _flatten(obj, prefix=""):
    for k, v in obj.items():
        assert "/" not in k, k
        if isinstance(v, dict):
            yield from _flatten(v, f"{prefix}{k}/")
        else:
            yield f"{prefix}{k}", v


def save_sharded(obj, stem):
    """Write ``obj`` (nested dicts, leaves: tensors / lists) as tests/golden/<stem>.NN.pt shards;
    earlier shards of that stem are replaced.  Returns the paths written."""
    os.makedirs(GOLDEN, exist_ok=True)
    for old in glob.glob(os.path.join(GOLDEN, f"{stem}.[0-9][0-9].pt")):
        os.remove(old)
    shards, size = [{}], 0
    for path, v in _flatten(obj):
        n = v.numel() * v.element_size() if isinstance(v, torch.Tensor) else 64 * len(v)
        assert n <= SHARD_BYTES, (path, n)
        if size + n > SHARD_BYTES:
            shards.append({})
            size = 0
        shards[-1][path] = v.clone() if isinstance(v, torch.Tensor) else v  # a clone: no shared storage saved whole
        size += n
    paths = []
    for i, s in enumerate(shards):
        paths.append(os.path.join(GOLDEN, f"{stem}.{i:02d}.pt"))
        torch.save(s, paths[-1])
    return paths


def load_sharded(stem):
    paths = sorted(glob.glob(os.path.join(GOLDEN, f"{stem}.[0-9][0-9].pt")))
    assert paths, f"no shards of {stem} under {GOLDEN}"
    out = {}
    for p in paths:
        for path, v in torch.load(p, weights_only=True).items():
            *dirs, leaf = path.split("/")
            d = out
            for k in dirs:
                d = d.setdefault(k, {})
            d[leaf] = v
    return out


def zero_dropout(module):
    """Train-mode parity without randomness: every nn.Dropout (block, MHA, FFN AND per-head) at 0."""
    for m in module.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return module
