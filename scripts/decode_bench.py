"""GPT-2 KV-cache decoding throughput on one MI355X (random-init weights, bf16, greedy).

For each batch size and for the eager and the hipGraph-replayed one-token step: one untimed
generate (GEMM autotuning of the prefill / decode shapes, graph capture) and a timed generate of
``--new`` tokens; the prompt pass alone is timed once after the first warm-up.  One JSON line per (batch, step form): prefill ms, ms per
decode step (generate time minus the prefill, over the steps), generated tokens/s over the batch.

    python scripts/decode_bench.py --model gpt2-small --batches 1,16,64 --prompt 128 --new 128

``--ragged``: the per-sequence path (``generate(prompt_lens=...)``) against the uniform captured step,
GPT-2-small at batch 64, prompt 128, 128 new tokens: (a) the uniform graph path and (b) the ragged
path with all lengths equal, alternated in one process, then (c) the ragged path with prompt lengths
spread evenly over 16 .. 512.  One JSON line per timed run and a summary line with the medians and
the (b) / (a) ratio.

    python scripts/decode_bench.py --ragged

``--sample``: sampled decoding (temperature 0.8, top_k 50, top_p 0.95) with the default sampler
(``sampler="torch"``: ATen ops after every replay) against the fused one captured with the step
(``sampler="native"``), the greedy captured step beside them, at batch 1, 16 and 64: the three
alternated in one process, three rounds.  One JSON line per timed run, then per batch a summary line
with the median ms per decode step of each and the torch / native ratio.

    python scripts/decode_bench.py --sample
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def ragged(m, model, B=64, prompt=128, new=128, rounds=3):
    """(a) uniform graph step, (b) ragged step at equal lengths, alternated; (c) ragged, lengths 16 .. 512."""
    from replicann_amd.models.blocks import KVCache
    dev = torch.device("cuda")
    V, nl = m.config.vocab_size, m.config.n_layer
    idx = torch.randint(0, V, (B, prompt), device=dev)
    spread = [16 + round(i * (512 - 16) / (B - 1)) for i in range(B)]
    idx_c = torch.randint(0, V, (B, max(spread)), device=dev)
    cases = {
        "uniform graph": (lambda: m.generate(idx, new, temperature=0, graph=True),
                          lambda: m.decode_step(idx, KVCache(nl, prompt + new))),
        "ragged graph, equal lengths": (
            lambda: m.generate(idx, new, prompt_lens=[prompt] * B, temperature=0, graph=True),
            lambda: m.decode_step(idx, KVCache(nl, prompt + new), lens=[prompt] * B)),
        "ragged graph, lengths 16..512": (
            lambda: m.generate(idx_c, new, prompt_lens=spread, temperature=0, graph=True),
            lambda: m.decode_step(idx_c, KVCache(nl, max(spread) + new), lens=spread)),
    }
    steps = {k: [] for k in cases}
    prefill = {}
    for name, (gen, pre) in cases.items():  # warm-up: GEMM tuning of every shape, graph capture
        gen()
        prefill[name] = min(_timed(pre)[0] for _ in range(2))
    a, b, c = cases
    for r in range(rounds):
        for name in (a, b):
            total, _ = _timed(cases[name][0])
            ms = (total - prefill[name]) / (new - 1) * 1e3
            steps[name].append(ms)
            print(json.dumps({"model": model, "batch": B, "prompt": prompt, "new_tokens": new, "case": name,
                              "round": r, "prefill_ms": round(prefill[name] * 1e3, 3),
                              "decode_ms_per_step": round(ms, 4),
                              "generated_tokens_per_s": round(B * new / total, 1)}), flush=True)
    for r in range(rounds):
        total, _ = _timed(cases[c][0])
        ms = (total - prefill[c]) / (new - 1) * 1e3
        steps[c].append(ms)
        print(json.dumps({"model": model, "batch": B, "prompt_lens": "16..512 evenly", "new_tokens": new, "case": c,
                          "round": r, "prefill_ms": round(prefill[c] * 1e3, 3), "decode_ms_per_step": round(ms, 4),
                          "generated_tokens_per_s": round(B * new / total, 1)}), flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in steps.items()}
    print(json.dumps({"summary": "median decode ms/step", **{k: round(v, 4) for k, v in med.items()},
                      "ragged_equal_over_uniform": round(med[b] / med[a], 4)}), flush=True)


def sample(m, model, batches, prompt=128, new=128, rounds=3):
    """sampler="torch" against sampler="native" (and greedy), alternated per round, per batch size."""
    from replicann_amd.models.blocks import KVCache
    from replicann_amd.ops import rng
    dev = torch.device("cuda")
    rng.manual_seed(0)
    sampled = dict(temperature=0.8, top_k=50, top_p=0.95, graph=True)
    for B in batches:
        idx = torch.randint(0, m.config.vocab_size, (B, prompt), device=dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        cases = {
            "greedy": lambda: m.generate(idx, new, temperature=0, graph=True),
            "torch": lambda: m.generate(idx, new, sampler="torch", generator=gen, **sampled),
            "native": lambda: m.generate(idx, new, sampler="native", **sampled),
        }
        for fn in cases.values():  # warm-up: GEMM tuning, graph capture
            fn()
        prefill = min(_timed(lambda: m.decode_step(idx, KVCache(m.config.n_layer, prompt + new)))[0] for _ in range(2))
        steps = {k: [] for k in cases}
        for r in range(rounds):
            for name, fn in cases.items():
                total, _ = _timed(fn)
                ms = (total - prefill) / (new - 1) * 1e3
                steps[name].append(ms)
                print(json.dumps({"model": model, "batch": B, "prompt": prompt, "new_tokens": new, "sampler": name,
                                  "round": r, "prefill_ms": round(prefill * 1e3, 3), "decode_ms_per_step": round(ms, 4),
                                  "generated_tokens_per_s": round(B * new / total, 1)}), flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in steps.items()}
        print(json.dumps({"summary": "median decode ms/step", "batch": B, **{k: round(v, 4) for k, v in med.items()},
                          "sampling_cost_torch_ms": round(med["torch"] - med["greedy"], 4),
                          "sampling_cost_native_ms": round(med["native"] - med["greedy"], 4),
                          "torch_over_native": round(med["torch"] / med["native"], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--ragged", action="store_true", help="uniform against ragged decode step (see above)")
    ap.add_argument("--sample", action="store_true", help="sampler='torch' against sampler='native' (see above)")
    a = ap.parse_args()
    from replicann_amd import _ext
    from replicann_amd.models.blocks import KVCache
    from replicann_amd.training import build_model
    from replicann_amd.tuning import load_committed
    if not _ext.available():
        raise RuntimeError(f"native extension missing: {_ext.load_error()}")
    dev = torch.device("cuda")
    load_committed(a.model)
    torch.manual_seed(0)
    m = build_model(a.model).to(dev)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    m.eval()
    if a.ragged:
        return ragged(m, a.model, prompt=a.prompt, new=a.new)
    if a.sample:
        return sample(m, a.model, [int(b) for b in a.batches.split(",")], prompt=a.prompt, new=a.new)
    for B in [int(b) for b in a.batches.split(",")]:
        idx = torch.randint(0, m.config.vocab_size, (B, a.prompt), device=dev)
        prefill = None
        for graph in (False, True):
            m.generate(idx, a.new, temperature=0, graph=graph)  # warm-up: tunes the decode GEMM shapes
            torch.cuda.synchronize()
            if prefill is None:  # the prompt pass alone, with its GEMM shapes tuned by the warm-up
                t0 = time.perf_counter()
                m.decode_step(idx, KVCache(m.config.n_layer, a.prompt + a.new))
                torch.cuda.synchronize()
                prefill = time.perf_counter() - t0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(idx, a.new, temperature=0, graph=graph)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
            step_ms = (total - prefill) / max(1, a.new - 1) * 1e3
            print(json.dumps({"model": a.model, "batch": B, "prompt": a.prompt, "new_tokens": a.new,
                              "decode_step": "hipGraph replay" if graph else "eager",
                              "prefill_ms": round(prefill * 1e3, 3), "decode_ms_per_step": round(step_ms, 3),
                              "generated_tokens_per_s": round(B * a.new / total, 1),
                              "out_shape": list(out.shape), "dtype": "bf16", "weights": "random init"}), flush=True)

if __name__ == "__main__":
    main()
