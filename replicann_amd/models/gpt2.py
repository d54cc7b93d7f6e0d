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
from dataclasses import dataclass

import torch
import torch.nn as nn

from .. import ops
from . import decoding
from .blocks import Fp8Slots, LayerNorm, PreLNBlock
from .decoding import DECODE_EOS_CHECK, DECODE_GRAPHS_MAX, DECODE_LEN_BUCKET, _sample  # noqa: F401  (re-exported)


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

    def _hidden_cached(self, idx, cache):
        """Final-LayerNorm output (B, T, n_embd) of ``idx`` (B, T) appended to ``cache``: the one
        cached pass, in whichever mode the cache is (prefill and every form of the one-token step)."""
        cache.begin_step(idx.shape[1])
        x = cache.embed(idx, self.wte, self.wpe)
        prev = None
        for i, blk in enumerate(self.h):
            x = blk(x, prev, cache=cache, layer=i)
            prev = blk.out_bias()
        return self.ln_f(x, producer_bias=prev)

    @torch.no_grad()
    def decode_step(self, idx, cache, lens=None):
        """Logits (B, vocab) of the LAST position of ``idx`` (B, T) appended at ``cache.pos``:
        prefill (T = prompt length) and one-token decode steps share this path.  In the cache's device
        modes (``decoding.KVCache``) a one-token step uses no host value: capturable as a hipGraph.

        ``lens`` (B host integers, 1 <= lens[b] <= T): ``idx`` is a right-padded batch of prompts of
        these lengths, prefilled into an empty cache.  The pass is the same causal one — causality
        makes every valid position right whatever the padding holds, and the padded positions' keys /
        values land at rows >= lens[b], which are never read and are overwritten as the row grows.
        The logits are those of each row's own last valid position, and the cache is left in
        per-sequence mode at position lens[b]: later ``decode_step(tok (B, 1), cache)`` calls advance
        every active row at its own position."""
        B, T = idx.shape
        if lens is not None:
            lens = decoding.host_lens("lens", lens, B, T)
            if cache.pos != 0 or cache.mode != "host":
                raise ValueError("a ragged prefill needs an empty cache (KVCache.reset())")
        h = self._hidden_cached(idx, cache)
        if lens is not None:
            cache.to_per_sequence(lens)
            # each row's own last valid position, gathered BEFORE the LM head: the head runs on B rows
            # (a cache shared by several samples per prompt has fanned out: its B rows' lengths are prefix_len)
            ends = cache.prefix_len if cache.shared else cache.pos_t
            last = h[torch.arange(B, device=h.device), ends - 1].unsqueeze(1).contiguous()
            return ops.linear(last, self.wte)[:, 0, : self.config.vocab_size]
        logits = ops.linear(h[:, -1:].contiguous(), self.wte)[:, 0, : self.config.vocab_size]
        cache.end_step(T)
        return logits

    def _window_logits(self, idx, cache):
        """Logits (B, T, vocab) of the window ``idx`` (B, T) written at each row's own cache position
        (per-sequence mode): the cached pass with the window attention, then the LM head on all B·T rows."""
        with cache.windowed():
            x = cache.embed(idx, self.wte, self.wpe)
            prev = None
            for i, blk in enumerate(self.h):
                x = blk(x, prev, cache=cache, layer=i)
                prev = blk.out_bias()
            h = self.ln_f(x, producer_bias=prev)
        return ops.linear(h, self.wte)[..., : self.config.vocab_size]

    @torch.no_grad()
    def decode_window(self, idx, cache):
        """Greedy token ids (B, T) after every position of the window ``idx`` (B, T): position i of row
        b is the model's next token given the row's cached prefix and ``idx[b, :i+1]``.  The window's
        keys / values are written at rows pos_t[b] .. pos_t[b] + T - 1 but the cache position does not
        move: the caller commits what it keeps with ``cache.advance(counts)``, and the rest is stale
        rows that the next step overwrites.  No host value is used: capturable as a hipGraph
        (``decoding.capture_window``)."""
        return self._window_logits(idx, cache).argmax(-1)

    @torch.no_grad()
    def decode_window_logits(self, idx, cache):
        """``decode_window`` returning the window's logits (B, T, vocab) instead of the greedy ids: what
        speculative sampling verifies the drafts against (``ops.speculative_verify``).  The cache is
        treated the same way."""
        return self._window_logits(idx, cache)

    def _device_position_step(self, tok, cache):
        """The one-token step ``tok`` (B, 1) → (B, vocab) logits that ``generate`` runs or captures."""
        return self.decode_step(tok, cache)

    def _capture_decode(self, cache, B, sampler=None):
        return decoding.capture_step(self, cache, B, sampler)

    # generation itself (the cache, the sampling loops, the captured-step registry): models/decoding.py
    generate = decoding.generate
    generate_batch = decoding.generate_batch

    def _decode_graphs(self):
        """The captured decode steps kept across ``generate`` calls (``decoding._GraphRegistry``)."""
        return decoding.registry(self)

    def clear_decode_graphs(self):
        decoding.registry(self).clear()

    def flops_per_token(self, T=None):
        """Training FLOPs per token (fwd+bwd): 6·N_matmul + attention (causal)."""
        c = self.config
        T = T or c.block_size
        n_mm = c.n_layer * 12 * c.n_embd**2 + c.vocab_size * c.n_embd
        attn = c.n_layer * 2 * 2 * T * c.n_embd * 0.5  # fwd, causal ≈ half
        return 6 * n_mm + 3 * attn

