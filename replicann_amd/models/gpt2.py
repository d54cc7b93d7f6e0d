"""GPT-2 (small 124M / medium 355M) — N19, the headline model of BASELINE.json.

Absent from the reference: built here from its standard
definition — learned token + position embeddings, pre-LN blocks with fused
c_attn (bias), true causal attention with scale 1/sqrt(head_dim), tanh-GELU
MLP, final LayerNorm and an LM head tied to the token embedding.

MI355X-specific choices:
  * the token-embedding / LM-head matrix is STORED with 50304 = 393·128 rows
    (MFMA tile multiple); rows ≥ 50257 are zero, never indexed, and masked out
    of the softmax by the fused cross-entropy (``n_valid_cols``), so the model
    is mathematically the 50257-vocab GPT-2;
  * the loss path never materialises fp32 logits: bf16 logits from the GEMM,
    log-sum-exp in the fused CE kernel, gradient written in place.
"""

from __future__ import annotations

import os
import weakref
from dataclasses import dataclass

import torch
import torch.nn as nn

from .. import ops
from .blocks import Fp8Slots, KVCache, LayerNorm, PreLNBlock


@dataclass(frozen=True)
class GPT2Config:
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    block_size: int = 1024
    vocab_size: int = 50257
    vocab_pad: int = 50304
    dropout: float = 0.0
    ln_eps: float = 1e-5
    fp8: bool = False  # fp8 e4m3 forward GEMMs in the transformer blocks ("fp8 weights" config)
    # fp8 also for the attention output projection (its input takes one delayed-scaling quantisation pass; c_attn /
    # c_fc take e4m3 straight from the LayerNorm kernel, the MLP c_proj from the gelu_q8 pass).  On by default since
    # round 5 call V: with the fp8 LM head 131.5 vs 133.6 ms/step, and over steps 40-49 of the 50-step trajectory the
    # loss stays within 0.5 % of bf16 (held-out loss 0.24 % behind, against 1.4 % with this projection in bf16); the
    # early descent (steps 6-9) deviates up to 8 % (profiles/gpt2m_fp8_proj_r5v.txt).  REPLICANN_FP8_PROJ=0: bf16
    # (None: resolved from the environment when the config is built, not at import time)
    fp8_proj: bool | None = None
    # fp8 LM head (fp8 models, training steps only; ops.loss._LinearXentFp8Fn): 1 = logits from e4m3 h · e4m3
    # wte, the loss gradient straight to e5m2 by the cross-entropy kernel, both head gradients on the fp8 GEMMs;
    # 2 = the same gradients with the logits GEMM kept in bf16 (the loss itself unquantised); 0 = bf16 head.
    # Default 1: GPT-2-medium-fp8 132.0 ms/step against 139.9 (bf16 head) and 166.0 (bf16) on one box; the
    # held-out loss after 50 steps is within 1.4 % of the bf16 model's (1.1 % with the bf16 head)
    # (profiles/gpt2m_fp8_head_r5op.txt)
    fp8_head: int | None = None
    # LM head + loss over row chunks of this many tokens (0: the whole batch at once).  Bounds the
    # logits buffer (rows x vocab_pad bf16: 6.6 GB at b64 x 1024) for long sequences / big batches
    ce_chunk: int = 0

    def __post_init__(self):
        if self.fp8_proj is None:
            object.__setattr__(self, "fp8_proj", os.environ.get("REPLICANN_FP8_PROJ", "1") == "1")
        if self.fp8_head is None:
            object.__setattr__(self, "fp8_head", int(os.environ.get("REPLICANN_FP8_HEAD", "1")))

    @staticmethod
    def small(**kw):
        return GPT2Config(**kw)

    @staticmethod
    def medium(**kw):
        return GPT2Config(n_layer=24, n_head=16, n_embd=1024, **kw)

    @staticmethod
    def tiny(**kw):
        """Test-size config (same code paths)."""
        d = dict(n_layer=2, n_head=4, n_embd=128, block_size=128, vocab_size=1000, vocab_pad=1024)
        d.update(kw)
        return GPT2Config(**d)


_DECODE_GRAPHS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
# captured decode steps kept per model (least recently used evicted first): each holds a KV cache of
# 2 · n_layer · B · length · n_embd elements (≈ 2.4 GB for GPT-2-small at B = 64, length 1024)
DECODE_GRAPHS_MAX = int(os.environ.get("REPLICANN_DECODE_GRAPHS", "4"))
DECODE_LEN_BUCKET = 64  # cache lengths are rounded up to this (capped at block_size): one graph per bucket
DECODE_EOS_CHECK = 8  # ragged generate: "has every row finished?" is asked of the device every this many steps


class GPT2(nn.Module):
    def __init__(self, config: GPT2Config | None = None, **kw):
        super().__init__()
        cfg = config or GPT2Config(**kw)
        self.config = cfg
        self.wte = nn.Parameter(torch.empty(cfg.vocab_pad, cfg.n_embd))
        self.wpe = nn.Parameter(torch.empty(cfg.block_size, cfg.n_embd))
        nn.init.normal_(self.wte, std=0.02)
        nn.init.normal_(self.wpe, std=0.01)
        with torch.no_grad():
            self.wte[cfg.vocab_size:].zero_()
        self.wte._rn_shared = True  # tied: embedding + LM head both contribute gradients ...
        self.wte._rn_direct_uses = 2  # ... each accumulated in place into the flat .grad
        self.h = nn.ModuleList(
            PreLNBlock(cfg.n_embd, cfg.n_head, causal=True, dropout=cfg.dropout, n_layer=cfg.n_layer,
                       eps=cfg.ln_eps, fp8=cfg.fp8, fp8_proj=cfg.fp8_proj)
            for _ in range(cfg.n_layer)
        )
        self.ln_f = LayerNorm(cfg.n_embd, cfg.ln_eps)
        # the fp8 LM head's scale slots (the weight is wte); absent unless fp8 and fp8_head
        self.head8 = Fp8Slots() if (cfg.fp8 and cfg.fp8_head > 0) else None

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        # a checkpoint of an fp8-head model loads into a model without the head's slots (fp8_head=0, a bf16
        # model): the slots are simply not needed — not an unexpected-key error
        if self.head8 is None:
            for k in [k for k in state_dict if k.startswith(prefix + "head8.")]:
                state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def num_params(self, non_embedding=False):
        n = sum(p.numel() for p in self.parameters())
        n -= (self.wte.shape[0] - self.config.vocab_size) * self.config.n_embd  # zero pad rows
        if non_embedding:
            n -= self.wpe.numel()
        return n

    def hidden(self, idx, fp8_head=None):
        """Final-LayerNorm output (B, T, n_embd); ``fp8_head``: the fp8 LM head's state, whose e4m3 input the
        LayerNorm kernel then writes as well."""
        x = ops.embedding(idx, self.wte, self.wpe)
        if self.config.dropout > 0 and self.training:
            x = ops.dropout(x, self.config.dropout, True)
        prev = prev8 = None
        for blk in self.h:
            x = blk(x, prev, prev_fp8=prev8)
            prev, prev8 = blk.out_bias(), blk.out_fp8()
        return self.ln_f(x, producer_bias=prev, fp8=fp8_head, producer_fp8=prev8)

    def forward(self, idx, targets=None):
        """idx (B, T) → logits (B, T, vocab_pad) [, mean CE loss when targets given].

        With ``targets`` only the loss is returned (logits are consumed in place).
        """
        fp8h = (self.head8.fp8_state if self.head8 is not None and targets is not None and self.training
                and torch.is_grad_enabled() and self.wte.is_cuda else None)
        if fp8h is not None:
            # decide here whether the fp8 head will run: otherwise ln_f would write (and roll the slot for) an
            # e4m3 copy nobody consumes (chunked head, or shapes the fp8 head does not take)
            rows = idx.numel()
            chunk = self.config.ce_chunk
            if (chunk and chunk < rows) or not ops.loss.fp8_head_ok(idx.new_empty((rows, self.config.n_embd),
                                                                                   device="meta"), self.wte):
                fp8h = None
        h = self.hidden(idx, fp8h)
        if targets is None:
            return ops.linear(h, self.wte)[..., : self.config.vocab_size]
        return ops.linear_cross_entropy(h, self.wte, targets, n_valid_cols=self.config.vocab_size,
                                        chunk_rows=self.config.ce_chunk, fp8=fp8h,
                                        fp8_logits=self.config.fp8_head != 2)

    @torch.no_grad()
    def decode_step(self, idx, cache, lens=None):
        """Logits (B, vocab) of the LAST position of ``idx`` (B, T) appended at ``cache.pos``:
        prefill (T = prompt length) and one-token decode steps share this path.

        ``lens`` (B host integers, 1 <= lens[b] <= T): ``idx`` is a right-padded batch of prompts of
        these lengths, prefilled into an empty cache.  The pass is the same causal one — causality
        makes every valid position right whatever the padding holds, and the padded positions' keys /
        values land at rows >= lens[b], which are never read and are overwritten as the row grows.
        The logits are those of each row's own last valid position, and the cache is left in
        per-sequence mode at position lens[b]: later ``decode_step(tok (B, 1), cache)`` calls advance
        every active row at its own position."""
        c = self.config
        T = idx.shape[1]
        if lens is not None:
            return self._ragged_prefill(idx, cache, lens)
        if cache.per_seq:
            if T != 1:
                raise ValueError("a cache in per-sequence mode takes one token per row and step")
            if cache.pos + 1 > cache.max_len:
                raise ValueError(f"KV cache full: {cache.pos} + 1 > {cache.max_len}")
            return self._device_position_step(idx, cache)
        x = ops.embedding(idx, self.wte, self.wpe[cache.pos: cache.pos + T])
        prev = None
        for i, blk in enumerate(self.h):
            x = blk(x, prev, cache=cache, layer=i)
            prev = blk.out_bias()
        h = self.ln_f(x, producer_bias=prev)
        cache.advance(T)
        return ops.linear(h[:, -1:].contiguous(), self.wte)[:, 0, : c.vocab_size]

    @torch.no_grad()
    def _ragged_prefill(self, idx, cache, lens):
        c = self.config
        B, T = idx.shape
        lens = [int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]
        if len(lens) != B or min(lens) < 1 or max(lens) > T:
            raise ValueError(f"lens must hold {B} values in [1, {T}], got {lens}")
        if cache.pos != 0 or cache.device_pos:
            raise ValueError("a ragged prefill needs an empty cache (KVCache.reset())")
        x = ops.embedding(idx, self.wte, self.wpe[:T])
        prev = None
        for i, blk in enumerate(self.h):
            x = blk(x, prev, cache=cache, layer=i)
            prev = blk.out_bias()
        h = self.ln_f(x, producer_bias=prev)
        cache.to_per_sequence(lens)
        # each row's own last valid position, gathered BEFORE the LM head: the head runs on B rows
        last = h[torch.arange(B, device=h.device), cache.pos_t - 1].unsqueeze(1).contiguous()
        return ops.linear(last, self.wte)[:, 0, : c.vocab_size]

    @torch.no_grad()
    def _device_position_step(self, tok, cache):
        """One-token decode step with every per-step value on the device (``KVCache`` device-position
        mode): capturable as a hipGraph.  Reads ``tok`` (B, 1), returns (B, vocab) logits, advances
        ``cache.pos_t``.  In per-sequence mode every row is appended, embedded and attended at its own
        position, and only the rows of ``cache.active`` advance."""
        c = self.config
        if cache.per_seq:
            # row b's position embedding is wpe[pos_t[b]]: the ids viewed as one sequence of B tokens
            x = ops.embedding(tok.view(1, -1), self.wte, self.wpe.index_select(0, cache.pos_t)).view(tok.shape[0], 1, -1)
        else:
            cache.mask.index_fill_(2, cache.pos_t, 0.0)
            x = ops.embedding(tok, self.wte, self.wpe.index_select(0, cache.pos_t))
        prev = None
        for i, blk in enumerate(self.h):
            x = blk(x, prev, cache=cache, layer=i)
            prev = blk.out_bias()
        h = self.ln_f(x, producer_bias=prev)
        logits = ops.linear(h, self.wte)[:, 0, : c.vocab_size]
        cache.step()
        return logits

    def _capture_decode(self, cache, B):
        """Record the one-token decode step as a hipGraph (after one eager warm-up that tunes the
        decode GEMM shapes); the caller writes the next token into ``tok`` and replays."""
        dev = self.wte.device
        tok = torch.zeros(B, 1, dtype=torch.long, device=dev)
        pos0 = cache.pos
        if cache.per_seq:  # ragged: the cache left its prefill in per-sequence mode
            pos_t0, lens0 = cache.pos_t.clone(), cache.lens.clone()

            def reset():  # the warm-up wrote each row's next (not yet valid) cache row and advanced: undo
                cache.pos_t.copy_(pos_t0)
                cache.lens.copy_(lens0)
                cache.pos = pos0
        else:
            cache.to_device_position()

            def reset():  # the warm-up wrote row pos0 and advanced the position: undo
                cache.pos_t.fill_(pos0)
                cache.mask[..., pos0:] = float("-inf")

        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._device_position_step(tok, cache)
        torch.cuda.current_stream(dev).wait_stream(side)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._device_position_step(tok, cache)
        reset()
        return graph, tok, out

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, *, temperature=1.0, top_k=None, top_p=None, generator=None, graph=None,
                 prompt_lens=None, eos_token_id=None, pad_token_id=None):
        """Autoregressive sampling with a KV cache: ``idx`` (B, T0) prompt → (B, T0 + max_new_tokens).
        ``temperature`` 0 = greedy; ``top_k`` / ``top_p`` restrict sampling.  One prefill pass over the prompt, then one-token steps whose
        attention reads the cached keys / values (no recomputation of the prefix).  ``graph``
        (default: on for GPU models): the one-token step is captured once as a hipGraph and replayed
        (per-step values live on the device), so a step costs its kernels, not ~130 host launches.

        Ragged batches / stopping (either of ``prompt_lens``, ``eos_token_id`` given): ``idx`` is
        right-padded, row b's prompt is ``idx[b, :prompt_lens[b]]`` (default: all of it) and whatever the
        padding holds is ignored.  A row is finished once it has emitted ``eos_token_id`` (kept in the
        output); from then on it emits ``pad_token_id`` (default: the EOS id, else 0) and its position
        stops.  Generation ends early once every row is finished (asked of the device every
        DECODE_EOS_CHECK steps).  Returns ``(tokens, lens)``: tokens (B, max(lens)), rows
        ``prompt_b ‖ generated_b`` right-padded with the pad id, and lens (B,) each row's total length."""
        c = self.config
        B, T0 = idx.shape
        if prompt_lens is not None or eos_token_id is not None:
            if top_p is not None and not 0.0 < top_p <= 1.0:
                raise ValueError(f"top_p must be in (0, 1], got {top_p}")
            return self._generate_ragged(idx, max_new_tokens, prompt_lens, eos_token_id, pad_token_id,
                                         dict(temperature=temperature, top_k=top_k, generator=generator, top_p=top_p),
                                         graph)
        if T0 + max_new_tokens > c.block_size:
            raise ValueError(f"prompt {T0} + {max_new_tokens} new tokens exceeds block_size {c.block_size}")
        if top_p is not None and not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {top_p}")
        use_graph = (self.wte.is_cuda if graph is None else graph) and max_new_tokens > 2
        was_training = self.training
        self.eval()
        try:
            L = T0 + max_new_tokens
            if use_graph:  # one captured step (and cache) serves every length of a bucket
                L = min(c.block_size, -(-L // DECODE_LEN_BUCKET) * DECODE_LEN_BUCKET)
            # the parameters' storage is part of the key: a graph reads them by address, so one captured
            # before a parameter was re-assigned (p.data = ...) must never be replayed
            sig = tuple(p.data_ptr() for p in self.parameters())
            key = (B, L, self.wte.dtype, self.wte.device, sig)
            graphs, entry = self._graph_entry(key, use_graph)
            if entry is not None:  # same batch / length as an earlier call: reuse its cache and graph
                cache = entry[0]
                cache.reset()
            else:
                cache = KVCache(c.n_layer, L)
            logits = self.decode_step(idx, cache)
            out = [idx]
            for i in range(max_new_tokens):
                nxt = _sample(logits.float(), temperature, top_k, generator, top_p)
                out.append(nxt)
                if i + 1 == max_new_tokens:
                    break
                if use_graph:
                    if entry is None:
                        while len(graphs) >= max(DECODE_GRAPHS_MAX, 1):  # bounded: evict the least recently used
                            graphs.pop(next(iter(graphs)))
                        entry = (cache, *self._capture_decode(cache, B))
                        graphs[key] = entry
                    elif not cache.device_pos:
                        cache.to_device_position()
                    _, g, tok, g_out = entry
                    tok.copy_(nxt)
                    g.replay()
                    logits = g_out
                else:
                    logits = self.decode_step(nxt, cache)
            return torch.cat(out, 1)
        finally:
            self.train(was_training)

    def _graph_entry(self, key, use_graph):
        """(registry, stored entry or None) for ``key``; entries captured on re-assigned parameters
        (key[4], the storage signature) are dropped, a hit becomes the most recently used."""
        graphs = self._decode_graphs()
        for k in [k for k in graphs if k[4] != key[4]]:
            del graphs[k]
        entry = graphs.pop(key, None) if use_graph else None
        if entry is not None:
            graphs[key] = entry
        return graphs, entry

    @torch.no_grad()
    def _generate_ragged(self, idx, max_new_tokens, prompt_lens, eos, pad, sample_kw, graph):
        c = self.config
        B, T0 = idx.shape
        dev = idx.device
        if prompt_lens is None:
            plens = [T0] * B
        else:
            plens = [int(n) for n in (prompt_lens.tolist() if torch.is_tensor(prompt_lens) else prompt_lens)]
        if len(plens) != B or min(plens) < 1 or max(plens) > T0:
            raise ValueError(f"prompt_lens must hold {B} values in [1, {T0}], got {plens}")
        Tm = max(plens)
        if max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be at least 1, got {max_new_tokens}")
        if Tm + max_new_tokens > c.block_size:
            raise ValueError(f"prompt {Tm} + {max_new_tokens} new tokens exceeds block_size {c.block_size}")
        if pad is None:
            pad = eos if eos is not None else 0
        use_graph = (self.wte.is_cuda if graph is None else graph) and max_new_tokens > 2
        was_training = self.training
        self.eval()
        try:
            L = min(c.block_size, -(-(Tm + max_new_tokens) // DECODE_LEN_BUCKET) * DECODE_LEN_BUCKET)
            sig = tuple(p.data_ptr() for p in self.parameters())
            key = (B, L, self.wte.dtype, self.wte.device, sig, "ragged")  # the mode last: k[4] stays the storage
            graphs, entry = self._graph_entry(key, use_graph)
            if entry is not None:
                cache = entry[0]
                cache.reset()
            else:
                cache = KVCache(c.n_layer, L)
            lens = torch.tensor(plens, dtype=torch.long, device=dev)  # each row's length so far
            # rows prompt ‖ generated, pad elsewhere (one spare column: a finished row's write lands in range)
            tokens = torch.full((B, Tm + max_new_tokens + 1), pad, dtype=torch.long, device=dev)
            keep = torch.arange(Tm, device=dev).unsqueeze(0) < lens.unsqueeze(1)
            tokens[:, :Tm] = torch.where(keep, idx[:, :Tm], tokens[:, :Tm])
            finished = torch.zeros(B, dtype=torch.bool, device=dev)
            logits = self.decode_step(idx[:, :Tm], cache, lens=plens)
            for i in range(max_new_tokens):
                nxt = _sample(logits.float(), **sample_kw)
                nxt = torch.where(finished.unsqueeze(1), torch.full_like(nxt, pad), nxt)  # finished rows emit pad
                tokens.scatter_(1, lens.unsqueeze(1), nxt)
                lens += ~finished
                if eos is not None:
                    finished |= nxt.squeeze(1) == eos
                if i + 1 == max_new_tokens:
                    break
                if eos is not None and (i + 1) % DECODE_EOS_CHECK == 0 and bool(finished.all()):
                    break  # the one host sync of the stop logic
                cache.active.copy_(~finished)  # finished rows stay where they are
                if use_graph:
                    if entry is None:
                        while len(graphs) >= max(DECODE_GRAPHS_MAX, 1):  # bounded: evict the least recently used
                            graphs.pop(next(iter(graphs)))
                        entry = (cache, *self._capture_decode(cache, B))
                        graphs[key] = entry
                    _, g, tok, g_out = entry
                    tok.copy_(nxt)
                    g.replay()
                    logits = g_out
                else:
                    logits = self._device_position_step(nxt, cache)
            return tokens[:, : int(lens.max())], lens
        finally:
            self.train(was_training)

    def generate_batch(self, prompts, max_new_tokens, **kw):
        """``generate`` for a list of 1-D token tensors of any lengths: pads them, runs the ragged
        path and returns a list of 1-D tensors ``prompt_b ‖ generated_b``, each trimmed to its length."""
        plens = [int(p.numel()) for p in prompts]
        if not plens or min(plens) < 1:
            raise ValueError("generate_batch needs at least one prompt, each of at least one token")
        idx = torch.zeros(len(prompts), max(plens), dtype=torch.long, device=self.wte.device)
        for b, p in enumerate(prompts):
            idx[b, : plens[b]] = p.to(idx.device)
        tokens, lens = self.generate(idx, max_new_tokens, prompt_lens=plens, **kw)
        return [tokens[b, :n] for b, n in enumerate(lens.tolist())]

    def _decode_graphs(self):
        """Captured decode steps kept across ``generate`` calls, keyed by (batch, cache length rounded
        up to DECODE_LEN_BUCKET, dtype, device, parameter storage[, "ragged" for the per-sequence step]):
        a serving loop captures once per
        (batch, length bucket).  At most DECODE_GRAPHS_MAX (REPLICANN_DECODE_GRAPHS, default 4) are
        kept, least recently used evicted first.  Each holds its KV cache (2 · n_layer · B · length ·
        n_embd elements); ``clear_decode_graphs`` frees them.  Kept
        outside the module's attributes (a weak-keyed registry), so copying / pickling the model
        never touches graph objects."""
        return _DECODE_GRAPHS.setdefault(self, {})

    def clear_decode_graphs(self):
        _DECODE_GRAPHS.pop(self, None)

    def flops_per_token(self, T=None):
        """Training FLOPs per token (fwd+bwd): 6·N_matmul + attention (causal)."""
        c = self.config
        T = T or c.block_size
        n_mm = c.n_layer * 12 * c.n_embd**2 + c.vocab_size * c.n_embd
        attn = c.n_layer * 2 * 2 * T * c.n_embd * 0.5  # fwd, causal ≈ half
        return 6 * n_mm + 3 * attn


def _sample(logits, temperature, top_k, generator, top_p=None):
    """(B, V) fp32 logits → (B, 1) next-token ids: greedy (temperature 0), else sampling from the
    temperature-scaled softmax restricted to the top-k logits and / or the smallest set of tokens
    whose probability mass reaches top_p (nucleus)."""
    if temperature == 0:
        return logits.argmax(-1, keepdim=True)
    logits = logits / temperature
    if top_k is not None and top_k < logits.shape[-1]:
        kth = torch.topk(logits, top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p is not None and top_p < 1.0:
        srt, idx = torch.sort(logits, dim=-1, descending=True)
        cum = torch.softmax(srt, -1).cumsum(-1)
        drop = cum - torch.softmax(srt, -1) >= top_p  # mass BEFORE a token already reaches top_p
        drop[..., 0] = False  # the most likely token always stays (top_p <= 0 would drop every token)
        srt = srt.masked_fill(drop, float("-inf"))
        logits = torch.full_like(logits, float("-inf")).scatter(-1, idx, srt)
    probs = torch.softmax(logits, -1)
    return torch.multinomial(probs, 1, generator=generator)
