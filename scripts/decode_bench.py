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

``--speculative``: what a round of speculative decoding costs, GPT-2-small drafting for GPT-2-medium
(``--model`` / ``--draft-model``), at batch 1, 16 and 64 after a prompt of ``--prompt`` tokens.  Per batch,
alternated in one process over three rounds of captured-graph replays: the target's and the draft's
ragged one-token step, and the target's window step at T = 5 and T = 9 on the window kernel and on
the composed path (the general attention under a (B, T, L + T) bias).  Then the per-layer kernel
times of ``attn_window`` against the one-query ``attn_decode``, the break-even mean accepted length
(at which a round of draft_k + 1 draft steps and one window step costs as much as the tokens it
yields cost one by one), and ``generate`` end to end with and without the draft — on RANDOM-INIT
weights, whose acceptance says nothing about trained models.  Every line is also appended to ``--out``.

    python scripts/decode_bench.py --speculative --out profiles/decode_speculative.txt
    python scripts/decode_bench.py --speculative --temperature 0.8 --out profiles/decode_speculative_sampling.txt

``--speculative --temperature T`` (T > 0): the sampled round of speculative SAMPLING instead: the draft's
K + 1 sampler launches, the verify launches of ``ops.speculative_verify`` and the composed ATen verification
of the same rule on the same logits (alternated in one process), then ``generate`` with and without the draft.

``--kv-fp8``: the captured one-token step over the bf16 KV cache against the one over the fp8 cache
(``generate(kv_dtype="fp8")``), GPT-2-small at batch 64, 128 new tokens after prompts of 128 and of 896 tokens (the
second fills the 1024-row bucket).  Per prompt the two graphs are alternated in one process after a warm-up of
each, three rounds of 128 replays from the prompt's position; one line per timed run, then the medians, the spread
of the rounds, each cache's bytes and the two criteria (prompt 896: fp8 faster by more than the spread; prompt 128:
at most 1.05x).  Then, inside captured graphs, the two attention kernels (24 calls walking the 12 layers' caches, so
that the rows come from memory as in the step) and the two QKV projections alone, and the relative L2 between fp8-cache and bf16-cache logits over 12 steps of the tests' tiny model
(reported, not gated: random weights).  Every line is also appended to ``--out``.

    python scripts/decode_bench.py --kv-fp8 --out profiles/decode_kv_fp8.txt
    rocprofv3 --kernel-trace --stats ... -- python scripts/decode_bench.py --kv-fp8 --prompts 896 --new 32   # per-kernel times

``--samples``: n samples per prompt over one shared prompt cache (``generate(num_samples=n)``) against the captured
ragged step on the repeated prompts (``generate(idx.repeat_interleave(n, 0), prompt_lens=...)``), GPT-2-small, 64 rows
per step as G x n = 1 x 64, 4 x 16 and 16 x 4, 128 new tokens after prompts of 128 and of 896 tokens.  The protocol
of ``--kv-fp8``: per case the two graphs alternated in one process after a warm-up of each, three rounds of 128
replays, medians and the spread of the rounds; then the prefill of G prompts against G · n, each cache's bytes, the
two criteria (1 x 64 at prompt 896: shared faster by more than the spread; prompt 128: every case at most 1.05x) and,
inside captured graphs that walk the 12 layers' caches, the attention of each step alone.

    python scripts/decode_bench.py --samples --out profiles/decode_shared_prefix.txt
"""

import argparse
import importlib
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


def _replay_ms(graph, n):
    t, _ = _timed(lambda: [graph.replay() for _ in range(n)])
    return t / n * 1e3


def _op_us(fn, calls=20, replays=10):
    """µs per call of ``fn`` inside a captured graph of ``calls`` of them (no launch gaps from the host)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    return _replay_ms(g, replays) / calls * 1e3


def speculative(m, d, names, batches, out_path, prompt=128, new=128, rounds=3, replays=30):
    from replicann_amd import ops
    from replicann_amd.models import decoding
    from replicann_amd.models.decoding import KVCache
    A = importlib.import_module("replicann_amd.ops.attention")  # the module: ops.attention is the function
    dev = torch.device("cuda")
    sink = open(out_path, "a") if out_path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    emit({"bench": "speculative decoding", "target": names[0], "draft": names[1], "prompt": prompt, "dtype": "bf16",
          "weights": "random init", "replays_per_timing": replays, "rounds": rounds})
    Ts = (5, 9)
    for B in batches:
        idx = torch.randint(0, m.config.vocab_size, (B, prompt), device=dev)
        length = -(-(prompt + new + max(Ts)) // decoding.DECODE_LEN_BUCKET) * decoding.DECODE_LEN_BUCKET
        caches, graphs = {}, {}
        for name, mod in (("target", m), ("draft", d)):
            c = caches[name] = KVCache(mod.config.n_layer, length)
            mod.decode_step(idx, c, lens=[prompt] * B)
            mod.decode_step(idx[:, :1], c)  # tunes the one-token GEMM shapes outside the capture
            c.restore((prompt, torch.full_like(c.pos_t, prompt), torch.full_like(c.pos_t, prompt + 1)))
            graphs[f"{name} one-token step"] = (decoding.capture_step(mod, c, B)[0], c)
        c = caches["target"]
        for T in Ts:
            for native in (True, False):
                A.WINDOW_NATIVE = native
                try:
                    m.decode_window(idx[:, :T], c)  # tunes the window GEMM shapes
                    graphs[f"window T={T} {'native' if native else 'composed'}"] = (decoding.capture_window(m, c, B, T)[0], c)
                finally:
                    A.WINDOW_NATIVE = True
        ms = {k: [] for k in graphs}
        for r in range(rounds):
            for k, (g, c) in graphs.items():
                snap = c.snapshot()
                g.replay()
                ms[k].append(_replay_ms(g, replays))
                c.restore(snap)  # the one-token steps moved the position
                emit({"batch": B, "case": k, "round": r, "ms_per_step": round(ms[k][-1], 4)})
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        summary = {"summary": "median ms per step", "batch": B, **{k: round(v, 4) for k, v in med.items()}}
        for T in Ts:
            comp = ms[f"window T={T} composed"]
            gain, spread = med[f"window T={T} composed"] - med[f"window T={T} native"], max(comp) - min(comp)
            summary[f"T={T} native gain ms"] = round(gain, 4)
            summary[f"T={T} composed spread ms"] = round(spread, 4)
            summary[f"T={T} kernel accepted"] = bool(gain > spread)
            # a round: T draft steps (draft_k + 1) and one window step, against (accepted + 1) one-token target steps
            cost = T * med["draft one-token step"] + med[f"window T={T} native"]
            summary[f"draft_k={T - 1} break-even mean accepted"] = round(cost / med["target one-token step"] - 1, 3)
        emit(summary)
        # the attention kernels alone, one layer: the window kernel against the one-query kernel
        H = m.config.n_head
        kv = torch.randn(B, length, 2, H, 64, device=dev).bfloat16()
        pos = torch.full((B,), prompt, device=dev)
        with torch.no_grad():
            q1 = torch.randn(B, 1, 3, H, 64, device=dev).bfloat16()
            rec = {"batch": B, "cached rows": prompt, "attn_decode64_k us": round(_op_us(
                lambda: ops.attention_decode(q1[:, :, 0], kv[:, :, 0], kv[:, :, 1], lens=pos + 1)), 2)}
            for T in (1,) + Ts:
                qT = torch.randn(B, T, 3, H, 64, device=dev).bfloat16()
                rec[f"attn_window T={T} us"] = round(_op_us(lambda: ops.attention_window(qT, kv, pos)), 2)
                A.WINDOW_NATIVE = False
                try:
                    rec[f"composed T={T} us"] = round(_op_us(lambda: ops.attention_window(qT, kv, pos)), 2)
                finally:
                    A.WINDOW_NATIVE = True
        emit(rec)
        del kv, graphs, caches
        # end to end, random-init weights: the acceptance is that of two unrelated random models
        runs = {"plain greedy": dict()}
        for T in Ts:
            runs[f"draft_k={T - 1}"] = dict(draft=d, draft_k=T - 1)
        for k, kw in runs.items():
            m.generate(idx, new, temperature=0, graph=True, **kw)  # warm-up: capture
            stats = {}
            total, _ = _timed(lambda: m.generate(idx, new, temperature=0, graph=True, **kw, **({"stats": stats} if kw else {})))
            rec = {"batch": B, "end to end": k, "weights": "random init", "new_tokens": new, "total_ms": round(total * 1e3, 2),
                   "generated_tokens_per_s": round(B * new / total, 1)}
            if kw:
                rec["rounds"] = stats["rounds"]
                rec["mean accepted per drafted"] = round(float(stats["accepted"].sum()) / max(1, int(stats["drafted"].sum())), 4)
            emit(rec)
        m.clear_decode_graphs()
        d.clear_decode_graphs()


def kv_fp8(m, model, out_path, B=64, prompts=(128, 896), new=128, rounds=3):
    """The captured step over a bf16 cache against the one over an fp8 cache (``--kv-fp8``)."""
    from replicann_amd import ops
    from replicann_amd.models import decoding
    from replicann_amd.models.decoding import KVCache
    from replicann_amd.models.gpt2 import GPT2, GPT2Config
    dev = torch.device("cuda")
    sink = open(out_path, "a") if out_path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    emit({"bench": "fp8 KV cache", "model": model, "batch": B, "new_tokens": new, "dtype": "bf16", "weights": "random init",
          "rounds": rounds, "replays_per_timing": new - 1})
    nl, H = m.config.n_layer, m.config.n_head
    for prompt in prompts:
        idx = torch.randint(0, m.config.vocab_size, (B, prompt), device=dev)
        length = min(m.config.block_size, -(-(prompt + new) // decoding.DECODE_LEN_BUCKET) * decoding.DECODE_LEN_BUCKET)
        graphs, nbytes = {}, {}
        for name, kvd in (("bf16 cache", None), ("fp8 cache", "fp8")):
            c = KVCache(nl, length, kvd)
            m.decode_step(idx, c)
            m.decode_step(idx[:, :1], c)  # tunes the one-token GEMM shapes outside the capture
            c.pos = prompt  # (the row that step wrote is overwritten by the first replay)
            cap = decoding.capture_step(m, c, B)
            graphs[name] = (cap[0], c, cap)  # the graph reads its token buffer by address: kept alive beside it
            nbytes[name] = sum(t.numel() * t.element_size() for t in c.kv + (c.kv_scale if kvd else []))
        ms = {k: [] for k in graphs}
        for r in range(rounds):
            for k, (g, c, _) in graphs.items():
                snap = c.snapshot()
                g.replay()
                ms[k].append(_replay_ms(g, new - 1))  # rows prompt .. prompt + new - 1
                c.restore(snap)
                emit({"prompt": prompt, "cache rows": length, "case": k, "round": r, "ms_per_step": round(ms[k][-1], 4)})
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        rec = {"summary": "median ms per captured step", "prompt": prompt, **{k: round(v, 4) for k, v in med.items()},
               "spread of the rounds ms": round(spread, 4), "fp8_over_bf16": round(med["fp8 cache"] / med["bf16 cache"], 4),
               **{f"{k} bytes": v for k, v in nbytes.items()},
               "cache bytes fp8_over_bf16": round(nbytes["fp8 cache"] / nbytes["bf16 cache"], 4)}
        if prompt >= 512:
            rec["criterion: fp8 faster by more than the spread"] = bool(med["bf16 cache"] - med["fp8 cache"] > spread)
        else:
            rec["criterion: fp8 at most 1.05x"] = bool(med["fp8 cache"] <= 1.05 * med["bf16 cache"])
        emit(rec)
        # the kernels alone at the prompt's row count: consecutive calls walk the 12 layers' caches (1.3 / 2.4 GB at
        # 1024 rows), as the step does, so that no call finds its rows in the 256 MiB last-level cache
        c8, cb = graphs["fp8 cache"][1], graphs["bf16 cache"][1]
        turn = [0]

        def layer():
            turn[0] = (turn[0] + 1) % nl
            return turn[0]
        pos = torch.full((B,), prompt, device=dev)
        lens = pos + 1
        blk = m.h[0].attn
        with torch.no_grad():
            qkv = torch.randn(B, 1, 3, H, 64, device=dev).bfloat16()
            h = torch.randn(B, 1, m.config.n_embd, device=dev).bfloat16()
            def bf16_attn():
                kv = cb.kv[layer()]
                return ops.attention_decode(qkv[:, :, 0], kv[:, :, 0], kv[:, :, 1], lens=lens)

            def fp8_attn():
                i = layer()
                return ops.attention_decode_kv8(qkv, c8.kv[i], c8.kv_scale[i], pos)

            emit({"prompt": prompt, "batch": B, "us per call inside a captured graph": "24 calls over the 12 layers' caches",
                  "attn_decode64_k (bf16 cache, lens)": round(_op_us(bf16_attn, calls=2 * nl), 2),
                  "attn_decode_kv8_k (fp8 cache, append included)": round(_op_us(fp8_attn, calls=2 * nl), 2),
                  "QKV GEMM with the append epilogue (linear_kv)": round(_op_us(
                      lambda: ops.linear_kv_append(h, blk.c_attn.weight, blk.c_attn.bias, cb.kv[0], pos[:1])), 2),
                  "QKV GEMM (linear)": round(_op_us(lambda: blk.c_attn(h)), 2)})
        del graphs, c8, cb
    # what the quantisation does to the logits: the tests' tiny model, 12 teacher-forced steps after a prompt of 20
    torch.manual_seed(0)
    tiny = GPT2(GPT2Config.tiny(n_embd=128, n_head=2, n_layer=2, block_size=128)).to(dev)
    for p in tiny.parameters():
        p.data = p.data.to(torch.bfloat16)
    tiny.eval()
    seq = torch.randint(0, 1000, (3, 32), device=dev)
    a, b = KVCache(2, 32), KVCache(2, 32, "fp8")
    errs = []
    for lo, hi in [(0, 20)] + [(t, t + 1) for t in range(20, 32)]:
        x, y = tiny.decode_step(seq[:, lo:hi], a).float(), tiny.decode_step(seq[:, lo:hi], b).float()
        errs.append(float((y - x).norm() / x.norm()))
    emit({"tiny model (random init), logits with the fp8 cache against the bf16 cache, relative L2": "not gated",
          "prefill": round(errs[0], 5), "steps": [round(e, 5) for e in errs[1:]], "max": round(max(errs[1:]), 5)})


def shared_prefix(m, model, out_path, shapes=((1, 64), (4, 16), (16, 4)), prompts=(128, 896), new=128, rounds=3):
    """n samples per prompt over one shared prompt cache against the captured ragged step on the repeated prompts
    (``--samples``)."""
    from replicann_amd import ops
    from replicann_amd.models import decoding
    from replicann_amd.models.decoding import KVCache
    dev = torch.device("cuda")
    sink = open(out_path, "a") if out_path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def bucket(x):
        return min(m.config.block_size, -(-x // decoding.DECODE_LEN_BUCKET) * decoding.DECODE_LEN_BUCKET)

    emit({"bench": "n samples per prompt over a shared prompt cache", "model": model, "new_tokens": new, "dtype": "bf16",
          "weights": "random init", "rounds": rounds, "replays_per_timing": new - 1})
    nl, H = m.config.n_layer, m.config.n_head
    for prompt in prompts:
        for G, n in shapes:
            B = G * n
            idx = torch.randint(0, m.config.vocab_size, (G, prompt), device=dev)
            rep = idx.repeat_interleave(n, 0)
            tok = torch.randint(0, m.config.vocab_size, (B, 1), device=dev)
            makers = {
                "repeated prompts": (lambda: KVCache(nl, bucket(prompt + new)), rep, B),
                "shared prompt": (lambda: KVCache(nl, bucket(prompt), samples=n, tail_len=bucket(new)), idx, G),
            }
            graphs, nbytes, prefill = {}, {}, {}
            for name, (make, ids, rows) in makers.items():
                c = make()
                m.decode_step(ids, c, lens=[prompt] * rows)
                snap = c.snapshot()
                m.decode_step(tok, c)  # tunes the one-token GEMM shapes outside the capture
                c.restore(snap)
                cap = decoding.capture_step(m, c, B)
                cap[1].copy_(tok)
                # (the graph reads its token buffer by address: the whole capture is kept alive beside it)
                graphs[name] = (cap[0], c, cap)
                nbytes[name] = sum(t.numel() * t.element_size() for t in c.kv + [p for p in c.prefix if p is not None])
                prefill[name] = min(_timed(lambda: m.decode_step(ids, make(), lens=[prompt] * rows))[0] for _ in range(2))
            ms = {k: [] for k in graphs}
            for r in range(rounds):
                for k, (g, c, _) in graphs.items():
                    snap = c.snapshot()
                    g.replay()
                    ms[k].append(_replay_ms(g, new - 1))  # rows prompt .. prompt + new - 1 / tail rows 0 .. new - 1
                    c.restore(snap)
                    emit({"prompt": prompt, "G x n": f"{G} x {n}", "case": k, "round": r,
                          "ms_per_step": round(ms[k][-1], 4)})
            med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
            spread = max(max(v) - min(v) for v in ms.values())
            a, b = "repeated prompts", "shared prompt"
            rec = {"summary": "median ms per captured step", "prompt": prompt, "G x n": f"{G} x {n}",
                   **{k: round(v, 4) for k, v in med.items()}, "spread of the rounds ms": round(spread, 4),
                   "shared_over_repeated": round(med[b] / med[a], 4),
                   **{f"{k} prefill ms": round(v * 1e3, 3) for k, v in prefill.items()},
                   **{f"{k} cache bytes": v for k, v in nbytes.items()},
                   "cache bytes shared_over_repeated": round(nbytes[b] / nbytes[a], 4)}
            if prompt >= 512 and (G, n) == (1, 64):
                rec["criterion: shared faster by more than the spread"] = bool(med[a] - med[b] > spread)
            if prompt < 512:
                rec["criterion: shared at most 1.05x"] = bool(med[b] <= 1.05 * med[a])
            emit(rec)
            # the kernels alone, half-way through the generation (new / 2 tail rows): consecutive calls walk the 12
            # layers' caches, as the step does, so that no call finds its rows in the last-level cache
            cs, cb = graphs[b][1], graphs[a][1]
            turn = [0]

            def layer():
                turn[0] = (turn[0] + 1) % nl
                return turn[0]
            plen = torch.full((G,), prompt, device=dev)
            none = torch.zeros_like(plen)
            pos = torch.full((B,), new // 2, device=dev)
            lens = torch.full((B,), prompt + new // 2 + 1, device=dev)
            with torch.no_grad():
                qkv = torch.randn(B, 1, 3, H, 64, device=dev).bfloat16()

                def plain_attn():
                    kv = cb.kv[layer()]
                    return ops.attention_decode(qkv[:, :, 0], kv[:, :, 0], kv[:, :, 1], lens=lens)

                def shared_attn(pl=plen):
                    i = layer()
                    return ops.attention_decode_prefix(qkv, cs.prefix[i], pl, cs.kv[i], pos)

                emit({"prompt": prompt, "G x n": f"{G} x {n}",
                      "us per call inside a captured graph": "24 calls over the 12 layers' caches, new / 2 rows generated",
                      "attn_decode64_k (repeated prompts, lens)": round(_op_us(plain_attn, calls=2 * nl), 2),
                      "prefix_partials64_k + prefix_tail_merge64_k (shared prompt, append included)":
                          round(_op_us(shared_attn, calls=2 * nl), 2),
                      "the same at prefix_len 0 (the partials launch returns at once: the tail + merge launch and the "
                      "boundary)": round(_op_us(lambda: shared_attn(none), calls=2 * nl), 2)})
            del graphs, cs, cb


def _composed_verify(tl, dl, drafts, temperature, top_k, top_p, u):
    """The accept / resample rule of ``ops.speculative_verify`` composed from ATen ops on the device (a sort, a
    softmax and a cumsum per row for the filters, as ``decoding._sample`` has them; inside tie groups it may
    differ from the kernel) — what verifying costs without the kernel.  No host value: capturable."""
    B, K1, V = tl.shape
    K = K1 - 1

    def probs(x):
        x = x.float() / temperature
        if top_k is not None and top_k < V:
            x = x.masked_fill(x < torch.topk(x, top_k, dim=-1).values[..., -1:], float("-inf"))
        if top_p is not None and top_p < 1.0:
            srt, idx = torch.sort(x, dim=-1, descending=True)
            sm = torch.softmax(srt, -1)
            drop = sm.cumsum(-1) - sm >= top_p
            drop[..., 0] = False
            x = torch.full_like(x, float("-inf")).scatter(-1, idx, srt.masked_fill(drop, float("-inf")))
        return torch.softmax(x, -1)

    p, q = probs(tl), probs(dl)
    at = drafts.unsqueeze(-1)
    pd, qd = p[:, :K].gather(2, at)[..., 0], q.gather(2, at)[..., 0]
    ok = (qd > 0) & (u[:, :K, 0] * qd < pd)
    res = (p[:, :K] - q).clamp_(min=0)
    res = torch.where(res.sum(-1, keepdim=True) > 0, res, p[:, :K])
    w = torch.cat([res, p[:, K:]], 1)
    cdf = w.cumsum(-1)
    cand = (cdf > u[..., 1:] * cdf[..., -1:]).to(torch.int8).argmax(-1)
    matched = ok.long().cumprod(1).sum(1)
    j = torch.arange(K1, device=tl.device).view(1, K1)
    a = matched.view(B, 1)
    padded = torch.cat([drafts, torch.zeros_like(drafts[:, :1])], 1)
    return torch.where(j < a, padded, torch.where(j == a, cand, torch.zeros_like(cand))), matched


def speculative_sampled(m, d, names, batches, out_path, temperature, prompt=128, new=128, rounds=3, K=4,
                        top_k=50, top_p=0.95):
    """What a SAMPLED speculative round costs (``--speculative --temperature T``): per batch, on the two models'
    own logits after the prompt, µs per call inside a captured graph of 20 calls, alternated over ``rounds``:
    the K + 1 native sampler launches of the draft tokens, the verify launches (``ops.speculative_verify``) and
    the composed ATen verification of the same rule on the same logits; then ``generate`` end to end."""
    from replicann_amd import ops
    from replicann_amd.models.decoding import KVCache
    from replicann_amd.ops import rng
    dev = torch.device("cuda")
    sink = open(out_path, "a") if out_path else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    emit({"bench": "speculative sampling", "target": names[0], "draft": names[1], "prompt": prompt, "dtype": "bf16",
          "weights": "random init", "draft_k": K, "temperature": temperature, "top_k": top_k, "top_p": top_p,
          "rounds": rounds})
    V = m.config.vocab_size
    for B in batches:
        idx = torch.randint(0, V, (B, prompt), device=dev)
        cache = KVCache(m.config.n_layer, prompt + 64)
        m.decode_step(idx, cache, lens=[prompt] * B)
        win = torch.randint(0, V, (B, K + 1), device=dev)
        tl = m.decode_window_logits(win, cache)  # (B, K+1, V): the padded LM head's slice
        dl = torch.empty(B, K, -(-V // 8) * 8, dtype=tl.dtype, device=dev)[..., :V]
        dl.copy_(d(win[:, :K])[..., :V])  # the draft model's logits on the same tokens
        drafts = torch.stack([ops.sample_logits(dl[:, i], temperature, top_k, top_p, seed_buf=rng.next_seed(dev))[0][:, 0]
                              for i in range(K)], 1)
        u = torch.rand(B, K + 1, 2, device=dev)
        seed = rng.next_seed(dev)
        cases = {
            f"{K + 1} sampler launches": lambda: [ops.sample_logits(tl[:, i], temperature, top_k, top_p, seed_buf=seed)
                                                   for i in range(K + 1)],
            "verify kernel": lambda: ops.speculative_verify(tl, dl, drafts, temperature, top_k, top_p, u=u,
                                                             check_drafts=False),
            "verify composed (ATen)": lambda: _composed_verify(tl, dl, drafts, temperature, top_k, top_p, u),
        }
        us = {k: [] for k in cases}
        for r in range(rounds):
            for k, fn in cases.items():
                us[k].append(_op_us(fn))
                emit({"batch": B, "case": k, "round": r, "us_per_call": round(us[k][-1], 2)})
        kt, mt = ops.speculative_verify(tl, dl, drafts, temperature, top_k, top_p, u=u, check_drafts=False)
        ct, cm = _composed_verify(tl, dl, drafts, temperature, top_k, top_p, u)
        emit({"summary": "median us per call", "batch": B, **{k: round(sorted(v)[len(v) // 2], 2) for k, v in us.items()},
              "composed spread us": round(max(us["verify composed (ATen)"]) - min(us["verify composed (ATen)"]), 2),
              "kernel and composed agree on matched": int((mt == cm).sum()), "of rows": B,
              "mean matched": round(float(mt.float().mean()), 3)})
        del cache, tl, dl
        runs = {"plain sampled (native)": dict(), f"draft_k={K}": dict(draft=d, draft_k=K)}
        kw0 = dict(temperature=temperature, top_k=top_k, top_p=top_p, sampler="native", graph=True)
        for k, kw in runs.items():
            m.generate(idx, new, **kw0, **kw)  # warm-up: capture
            stats = {}
            total, _ = _timed(lambda: m.generate(idx, new, **kw0, **kw, **({"stats": stats} if kw else {})))
            rec = {"batch": B, "end to end": k, "weights": "random init", "new_tokens": new, "total_ms": round(total * 1e3, 2),
                   "generated_tokens_per_s": round(B * new / total, 1)}
            if kw:
                rec["rounds"] = stats["rounds"]
                rec["mean accepted per drafted"] = round(float(stats["accepted"].sum()) / max(1, int(stats["drafted"].sum())), 4)
            emit(rec)
        m.clear_decode_graphs()
        d.clear_decode_graphs()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="gpt2-small")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--ragged", action="store_true", help="uniform against ragged decode step (see above)")
    ap.add_argument("--sample", action="store_true", help="sampler='torch' against sampler='native' (see above)")
    ap.add_argument("--speculative", action="store_true", help="the cost of a speculative round (see above)")
    ap.add_argument("--kv-fp8", action="store_true", help="the captured step over an fp8 KV cache against the bf16 one (see above)")
    ap.add_argument("--samples", action="store_true",
                    help="n samples per prompt over a shared prompt cache against the repeated prompts (see above)")
    ap.add_argument("--prompts", default="128,896",
                    help="--kv-fp8, --samples: the prompt lengths (one alone for a kernel trace)")
    ap.add_argument("--draft-model", default="gpt2-small")
    ap.add_argument("--out", default="", help="--speculative, --kv-fp8: also append every line to this file")
    ap.add_argument("--temperature", type=float, default=0.0,
                    help="--speculative: > 0 measures the SAMPLED round instead (top_k 50, top_p 0.95, draft_k 4): the "
                         "sampler launches, the verify kernel against the composed ATen verification, and generate")
    a = ap.parse_args()
    if a.speculative and a.model == "gpt2-small":
        a.model = "gpt2-medium"  # the default pair: small drafts for medium
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
    if a.speculative:
        load_committed(a.draft_model)
        torch.manual_seed(1)
        d = build_model(a.draft_model).to(dev)
        for p in d.parameters():
            p.data = p.data.to(torch.bfloat16)
        d.eval()
        with torch.no_grad():
            if a.temperature > 0:
                return speculative_sampled(m, d, (a.model, a.draft_model), [int(b) for b in a.batches.split(",")],
                                           a.out, a.temperature, prompt=a.prompt, new=a.new)
            return speculative(m, d, (a.model, a.draft_model), [int(b) for b in a.batches.split(",")], a.out,
                               prompt=a.prompt, new=a.new)
    if a.kv_fp8:
        with torch.no_grad():
            return kv_fp8(m, a.model, a.out, prompts=[int(p) for p in a.prompts.split(",")], new=a.new)
    if a.samples:
        with torch.no_grad():
            return shared_prefix(m, a.model, a.out, prompts=[int(p) for p in a.prompts.split(",")], new=a.new)
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
