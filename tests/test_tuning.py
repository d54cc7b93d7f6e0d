"""GEMM autotuner table round trip (gemm_tuning_table -> gemm_tuning_load), the mechanism that makes
every data-parallel rank adopt rank 0's measured kernel choices (Trainer._tune).  CPU-only: the
table ops have no tensor arguments; needs the built extension."""

import json
import os
from pathlib import Path

import pytest
import torch

SO = Path(__file__).resolve().parent.parent / "replicann_amd" / "_C.so"


@pytest.mark.skipif(not SO.exists(), reason="extension not built")
def test_tuning_table_round_trip():
    torch.ops.load_library(str(SO))
    entries = [dict(M=768, N=768, K=65536, ta=1, tb=0, act=0, f32=0, **{"as": 1}, epi=8, cfg=0, split=14),
               dict(M=65536, N=3072, K=768, ta=0, tb=1, act=5, f32=0, **{"as": 0}, epi=1, cfg=9, split=1)]
    assert torch.ops.replicann.gemm_tuning_load(json.dumps(entries, separators=(",", ":"))) == 2
    table = json.loads(torch.ops.replicann.gemm_tuning_table())
    for e in entries:
        assert e in table
    # loading a rank-0 table overrides a local pick for the same key
    e2 = dict(entries[1], cfg=1)
    assert torch.ops.replicann.gemm_tuning_load(json.dumps([e2], separators=(",", ":"))) == 1
    assert e2 in json.loads(torch.ops.replicann.gemm_tuning_table())


BASE = [9, 1, 6, 0, 2, 8]
SPLITS12 = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16]


def _candidates(M, N, K, *, ta=False, tb=False, act=0, out_fp32=False, accumulate=False, split_k=0, bias=False,
                residual=False, alpha=False, bias_grad=False):
    flat = torch.ops.replicann.gemm_candidates(M, N, K, ta, tb, act, out_fp32, accumulate, split_k, bias, residual,
                                               alpha, bias_grad, N)
    return list(zip(flat[0::2], flat[1::2]))


@pytest.mark.skipif(not SO.exists(), reason="extension not built")
def test_gemm_candidates_are_what_the_tuner_times():
    """The (cfg, split) pairs the autotuner walks, in its order (csrc/include/gemm_plan.h), with the
    library candidate off (its default)."""
    assert os.environ.get("REPLICANN_GEMM_LIB", "0") != "1", "expectations are for REPLICANN_GEMM_LIB unset"
    torch.ops.load_library(str(SO))
    fwd = dict(tb=True, bias=True)
    # Linear forward with a bias: the one-wave-per-SIMD config 11 joins the six tile configs
    assert _candidates(4096, 768, 768, **fwd) == [(c, 1) for c in BASE + [11]]
    # ... but not with a residual, nor with bias and alpha together
    assert _candidates(4096, 768, 768, residual=True, **fwd) == [(c, 1) for c in BASE]
    assert _candidates(4096, 768, 768, alpha=True, **fwd) == [(c, 1) for c in BASE]
    # decode rows: the skinny config 10 last; one row past its limit, gone
    assert _candidates(8, 2304, 768, **fwd) == [(c, 1) for c in BASE + [11, 10]]
    assert 10 not in [c for c, _ in _candidates(65, 2304, 768, **fwd)]
    # weight gradient with the split left to the tuner: every tile config over the 12-entry split list
    wgrad = _candidates(768, 3072, 65536, ta=True, accumulate=True, out_fp32=True, split_k=-1)
    assert wgrad == [(c, s) for c in BASE for s in SPLITS12] and len(wgrad) == 72
    # a short K stops each config's splits at the first one that leaves fewer than 256 per slab
    assert _candidates(768, 768, 1024, ta=True, split_k=-1) == [(c, s) for c in BASE for s in (1, 2, 3, 4)]
    # fused activation backward with the bias gradient: 256x192 (cfg 6) cannot emit column partials
    assert _candidates(4096, 3072, 768, act=6, bias_grad=True) == [(c, 1) for c in (9, 1, 0, 2, 8)]
    # config 11 wants whole 64-deep K tiles, at least two
    for K, has11 in ((64, False), (128, True), (200, False)):
        assert (11 in [c for c, _ in _candidates(4096, 768, K, **fwd)]) == has11, K


@pytest.mark.skipif(not SO.exists(), reason="extension not built")
def test_committed_tables_load_completely():
    """Every committed per-model table (replicann_amd/tuning/gemm_<model>.json) is loaded entry for
    entry by the native loader (load_committed raises on a partial parse)."""
    from replicann_amd import tuning

    torch.ops.load_library(str(SO))
    models = [p.stem[len("gemm_"):] for p in tuning.DIR.glob("gemm_*.json")]
    assert {"gpt2-small", "gpt2-medium", "gpt2-medium-fp8", "vit-b16", "resnet18"} <= set(models)
    for m in models:
        rows = json.loads(tuning.table_path(m).read_text())
        assert rows and tuning.load_committed(m) == len(rows)
        table = json.loads(torch.ops.replicann.gemm_tuning_table())
        for r in rows:
            assert {k: r[k] for k in tuning.KEYS} in table
