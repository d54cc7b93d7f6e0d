"""T1 reference parity: same signatures, state_dict layout and
forward outputs as the reference's ``replicann`` package (fp32, eval mode, CPU).

The reference side is recorded, not imported: ``scripts/gen_reference_golden.py`` ran the
reference's own code and stored its signatures, weights (its own init), seeded inputs and outputs
in ``tests/golden/ref_cpu_parity.pt``, so these tests need nothing outside the repository."""

import inspect
import os

import pytest
import torch

import replicann_amd.arch.transformer as T
import replicann_amd.nn.attention as A

ATOL = 2e-5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cpu_parity.pt")


@pytest.fixture(scope="module")
def gold():
    return torch.load(GOLD, weights_only=True)


def _copy(ref_sd, new_mod):
    new_mod.load_state_dict(ref_sd, strict=True)


def _sig(f):
    return [[p.name, int(p.kind), repr(p.default)] for p in inspect.signature(f).parameters.values()]


def _same_keys(sa, b):
    sb = b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    for k in sa:
        assert sa[k].shape == sb[k].shape, k
        assert sa[k].dtype == sb[k].dtype, k


def _close(a, b):
    torch.testing.assert_close(a, b, atol=ATOL, rtol=1e-5)


@pytest.mark.parametrize("name", ["SelfAttentionHead", "CrossAttentionHead", "MultiheadSelfAttention",
                                  "MultiheadCrossAttention"])
def test_attention_signatures(gold, name):
    r = gold["signatures"][name]
    n = getattr(A, name)
    assert r["init"] == _sig(n.__init__)
    assert r["forward"] == _sig(n.forward)


@pytest.mark.parametrize("name", ["TransformerEncoder", "TransformerDecoder", "TransformerCrossDecoder"])
def test_block_signatures(gold, name):
    r = gold["signatures"][name]
    n = getattr(T, name)
    assert r["init"] == _sig(n.__init__)
    assert r["forward"] == _sig(n.forward)


@pytest.mark.parametrize("H,E", [(2, 8), (3, 12), (4, 10)])
def test_encoder_parity(gold, H, E):
    r = gold[f"encoder_h{H}_e{E}"]
    n = T.TransformerEncoder(H, E).eval()
    _same_keys(r["sd"], n)
    _copy(r["sd"], n)
    _close(n(r["x"]), r["y"])
    assert ("kv_y" in r) == (E % H == 0)
    if E % H == 0:  # the reference's return_kv path crashes otherwise (z width != E)
        yn, kn, vn = n(r["x"], return_kv=True)
        for a, b in ((yn, r["kv_y"]), (kn, r["kv_k"]), (vn, r["kv_v"])):
            _close(a, b)
    # unbatched and extra leading dims
    assert r["x2"].shape == (5, E) and r["x4"].shape == (2, 2, 5, E)
    _close(n(r["x2"]), r["y2"])
    _close(n(r["x4"]), r["y4"])


def test_encoder_bias_options(gold):
    r = gold["encoder_bias_options"]
    kw = dict(ffn_bias=False, ffn_hidden_size=20, head_bias=True, proj_bias=False, p_dropout=0.0)
    n = T.TransformerEncoder(2, 8, **kw).eval()
    _same_keys(r["sd"], n)
    _copy(r["sd"], n)
    _close(n(r["x"]), r["y"])


def test_decoder_parity_noncausal_mask(gold):
    r = gold["decoder"]
    n = T.TransformerDecoder(2, 8, context_size=16).eval()
    _same_keys(r["sd"], n)
    assert list(n.state_dict())[0] == "_attn_mask"
    _copy(r["sd"], n)
    x = r["x"]
    _close(n(x), r["y"])
    # Q2: the additive 0/1 mask is NOT causal — a future token changes position 0
    x2 = x.clone()
    x2[:, -1] += 1.0
    assert not torch.allclose(n(x)[:, 0], n(x2)[:, 0])


def test_decoder_bf16_buffer_accepted():
    # Q3 deviation: the reference raises TypeError after .to(bf16); we accept any float mask
    n = T.TransformerDecoder(2, 8, context_size=8).eval().to(torch.bfloat16)
    y = n(torch.randn(1, 4, 8, dtype=torch.bfloat16))
    assert y.dtype == torch.bfloat16 and torch.isfinite(y.float()).all()


def test_cross_decoder_parity(gold):
    r = gold["cross_decoder"]
    ne = T.TransformerEncoder(2, 8).eval()
    nd = T.TransformerCrossDecoder(2, 8, context_size=12).eval()
    _same_keys(r["dec_sd"], nd)
    _copy(r["enc_sd"], ne)
    _copy(r["dec_sd"], nd)
    _, kn, vn = ne(r["src"], return_kv=True)
    _close(kn, r["k"])
    _close(vn, r["v"])
    _close(nd(r["tgt"], kn, vn), r["y"])


def test_heads_parity(gold):
    r = gold["self_head"]
    n = A.SelfAttentionHead(8, 4).eval()
    _same_keys(r["sd"], n)
    _copy(r["sd"], n)
    x = r["x"]
    _close(n(x), r["y"])
    zn, kn, vn = n(x, None, True)
    _close(zn, r["kv_z"])
    _close(kn, r["kv_k"])
    _close(vn, r["kv_v"])
    assert n.embeddings_size == r["embeddings_size"] and n.head_size == r["head_size"]
    r = gold["cross_head"]
    n = A.CrossAttentionHead(8, 4).eval()
    _copy(r["sd"], n)
    _close(n(r["x"], r["k"], r["v"]), r["y"])


def test_masks(gold):
    r = gold["masks"]
    n = A.MultiheadSelfAttention(2, 4, 8).eval()
    _copy(r["sd"], n)
    x = r["x"]
    assert r["bmask"].dtype == torch.bool and torch.equal(r["bmask"], torch.triu(torch.ones(6, 6, dtype=torch.bool), 1))
    _close(n(x, mask=r["bmask"]), r["y_bmask"])
    assert r["fmask"].shape == (2, 6, 6) and r["fmask"].dtype == torch.float32
    _close(n(x, mask=r["fmask"]), r["y_fmask"])
    with pytest.raises(TypeError):
        n(x, mask=torch.ones(6, 6, dtype=torch.int32))


def test_mhca_parity(gold):
    r = gold["mhca"]
    n = A.MultiheadCrossAttention(2, 4, 8).eval()
    _same_keys(r["sd"], n)
    _copy(r["sd"], n)
    x, k, v = r["x"], r["k"], r["v"]
    _close(n(x, k, v), r["y"])
    # Q6: return_kv works here (reference crashes)
    z, kk, vv = n(x, k, v, return_kv=True)
    assert z.shape == (2, 5, 8) and kk.shape == k.shape


def test_head_dropout_quirk():
    # Q4: head dropout stays 0.1 regardless of the block's p_dropout
    n = T.TransformerEncoder(2, 8, p_dropout=0.0)
    ps = [m.p for m in n.modules() if isinstance(m, torch.nn.Dropout)]
    assert ps == [0.1, 0.1, 0.0, 0.0]


def test_properties(gold):
    r = gold["properties"]
    n = T.TransformerEncoder(3, 12)
    for p in ("embedding_size", "head_size", "n_heads"):
        assert getattr(n, p) == r[p]
    assert n._ffn.hidden_size == r["ffn_hidden_size"]
    assert n._attn.head_size == r["attn_head_size"]


def test_train_mode_backward_runs():
    n = T.TransformerDecoder(2, 8, context_size=8).train()
    y = n(torch.randn(2, 8, 8))
    y.sum().backward()
    assert all(p.grad is not None for p in n.parameters())


def test_compat_import_paths():
    from replicann.arch.transformer import TransformerEncoder
    from replicann.nn.attention import MultiheadSelfAttention

    assert TransformerEncoder is T.TransformerEncoder
    assert MultiheadSelfAttention is A.MultiheadSelfAttention
