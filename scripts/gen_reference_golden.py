"""Record the REFERENCE's signatures, state_dict layouts and fp32 CPU outputs for
tests/test_reference_parity.py, so those tests need no copy of the reference.

Imports the reference implementation read-only from REFERENCE_SRC (a directory holding its
``replicann`` package), builds each block with its own random init under a fixed seed, runs it
in eval mode on seeded inputs and saves weights, inputs and outputs to
tests/golden/ref_cpu_parity.pt (tensors, strings and numbers only: loaded with weights_only=True).

    python scripts/gen_reference_golden.py REFERENCE_SRC
"""

import importlib
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ref_cpu_parity.pt")

ATTENTION = ["SelfAttentionHead", "CrossAttentionHead", "MultiheadSelfAttention", "MultiheadCrossAttention"]
BLOCKS = ["TransformerEncoder", "TransformerDecoder", "TransformerCrossDecoder"]
ENCODER_CASES = [(2, 8), (3, 12), (4, 10)]
BIAS_KW = dict(ffn_bias=False, ffn_hidden_size=20, head_bias=True, proj_bias=False, p_dropout=0.0)


def load_reference(src):
    for k in [k for k in sys.modules if k == "replicann" or k.startswith("replicann.")]:
        del sys.modules[k]
    sys.path.insert(0, src)
    try:
        att = importlib.import_module("replicann.nn.attention")
        tr = importlib.import_module("replicann.arch.transformer")
    finally:
        sys.path.remove(src)
    return att, tr


def sig(f):
    """A signature as plain data: (name, kind, repr(default)) per parameter."""
    return [[p.name, int(p.kind), repr(p.default)] for p in inspect.signature(f).parameters.values()]


def sd(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


def rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@torch.no_grad()
def main(src):
    att, tr = load_reference(src)
    g = {"signatures": {}}
    for mod, names in ((att, ATTENTION), (tr, BLOCKS)):
        for n in names:
            c = getattr(mod, n)
            g["signatures"][n] = {"init": sig(c.__init__), "forward": sig(c.forward)}

    for H, E in ENCODER_CASES:
        torch.manual_seed(0)
        r = tr.TransformerEncoder(H, E).eval()
        x, x2, x4 = rand(10, 3, 7, E), rand(11, 5, E), rand(12, 2, 2, 5, E)
        c = {"sd": sd(r), "x": x, "y": r(x), "x2": x2, "y2": r(x2), "x4": x4, "y4": r(x4)}
        if E % H == 0:  # the reference's return_kv path crashes otherwise (z width != E)
            c["kv_y"], c["kv_k"], c["kv_v"] = r(x, return_kv=True)
        g[f"encoder_h{H}_e{E}"] = c

    torch.manual_seed(1)
    r = tr.TransformerEncoder(2, 8, **BIAS_KW).eval()
    x = rand(20, 2, 6, 8)
    g["encoder_bias_options"] = {"sd": sd(r), "x": x, "y": r(x)}

    torch.manual_seed(2)
    r = tr.TransformerDecoder(2, 8, context_size=16).eval()
    x = rand(30, 3, 9, 8)
    g["decoder"] = {"sd": sd(r), "x": x, "y": r(x)}

    torch.manual_seed(3)
    re = tr.TransformerEncoder(2, 8).eval()
    rd = tr.TransformerCrossDecoder(2, 8, context_size=12).eval()
    s, t = rand(40, 2, 10, 8), rand(41, 2, 6, 8)
    _, k, v = re(s, return_kv=True)
    g["cross_decoder"] = {"enc_sd": sd(re), "dec_sd": sd(rd), "src": s, "tgt": t, "k": k, "v": v, "y": rd(t, k, v)}

    torch.manual_seed(4)
    r = att.SelfAttentionHead(8, 4).eval()
    x = rand(50, 2, 5, 8)
    z, k, v = r(x, None, True)
    g["self_head"] = {"sd": sd(r), "x": x, "y": r(x), "kv_z": z, "kv_k": k, "kv_v": v,
                      "embeddings_size": int(r.embeddings_size), "head_size": int(r.head_size)}
    r = att.CrossAttentionHead(8, 4).eval()
    x, k, v = rand(51, 2, 5, 8), rand(52, 2, 7, 4), rand(53, 2, 7, 4)
    g["cross_head"] = {"sd": sd(r), "x": x, "k": k, "v": v, "y": r(x, k, v)}

    torch.manual_seed(5)
    r = att.MultiheadSelfAttention(2, 4, 8).eval()
    x, fmask = rand(60, 2, 6, 8), rand(61, 2, 6, 6)
    bmask = torch.triu(torch.ones(6, 6, dtype=torch.bool), 1)
    g["masks"] = {"sd": sd(r), "x": x, "bmask": bmask, "y_bmask": r(x, mask=bmask),
                  "fmask": fmask, "y_fmask": r(x, mask=fmask)}

    torch.manual_seed(6)
    r = att.MultiheadCrossAttention(2, 4, 8).eval()
    x, k, v = rand(70, 2, 5, 8), rand(71, 2, 7, 8), rand(72, 2, 7, 8)
    g["mhca"] = {"sd": sd(r), "x": x, "k": k, "v": v, "y": r(x, k, v)}

    r = tr.TransformerEncoder(3, 12)
    g["properties"] = {"embedding_size": int(r.embedding_size), "head_size": int(r.head_size),
                       "n_heads": int(r.n_heads), "ffn_hidden_size": int(r._ffn.hidden_size),
                       "attn_head_size": int(r._attn.head_size)}

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(g, OUT)
    torch.load(OUT, weights_only=True)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB): {sorted(g)}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
