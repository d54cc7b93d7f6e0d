"""Incremental decoding: everything that is generation, not model.

``KVCache`` owns everything that depends on its mode; ``generate`` is the sampling loop (uniform or
ragged) over one ``_StepDriver``, which resolves the cache and runs the one-token step eagerly or as
a hipGraph kept in the model's ``_GraphRegistry``.  The model (``models/gpt2.py``) keeps the pass.
With a draft model, ``generate`` is speculative decoding (``_speculative_loop``): the draft's one-token
steps, the target's window step (``_WindowDriver``, ``capture_window``) and ``accept`` — greedy, or with
``sampler="native"`` speculative sampling (``ops.speculative_verify`` decides what ``accept`` commits).
"""

from __future__ import annotations

import contextlib
import os
import weakref

import torch

from .. import ops
from ..ops import rng


class KVCache:
    """Per-layer key / value buffer for incremental decoding, (B, max_len, 2, H, D), allocated on
    first use in the dtype / device of the keys (one HBM allocation per layer for the whole
    generation; an append is one row copy, the attention reads strided key / value views).

    ``mode`` says where the position lives and what the attention reads:
      * ``"host"`` (a new or ``reset()`` cache; prefills): the host integer ``pos``; appends are slice
        copies and the attention is the causal one over rows < pos + T.
      * ``"device"`` (a captured step, ``generate(graph=True)``): the write row is the 1-element
        device tensor ``pos_t`` and the attention reads the whole buffer under the additive key
        ``mask`` (1, 1, max_len), 0 for written rows, -inf past them — no host value per step.
      * ``"per_seq"`` (ragged batches, ``decode_step(lens=...)``): ``pos_t`` (B,) is each row's write
        row, ``lens = pos_t + 1`` the key count its attention reads once this step's row is appended
        (no mask: rows past it are never read), ``active`` (B,) 0 / 1 the rows that advance (0: a
        finished row stays where it is).  ``pos`` is max over the rows: an upper bound.
        Only this mode has the window step (``windowed`` / ``window`` / ``advance`` / ``set_rows``): T
        tokens per row written and attended at each row's own position, committed separately.
    A captured step reads the device tensors by address, so each is allocated once per cache and kept
    through ``reset()`` and every mode change (the per-sequence triple: until the batch size changes).

    ``kv_dtype="fp8"`` (default None: the cache above, untouched): ``kv[layer]`` is uint8 (B, max_len, 2, H, D)
    OCP e4m3 bytes and ``kv_scale[layer]`` fp32 (B, max_len, 2, H) their scales, one power of two per head row
    (``ops.kv8``: about half the bytes).  The attention layer hands the packed projection output to ``step8``:
    a one-token step in any mode is one ``ops.attention_decode_kv8`` — append and attention — at the mode's own
    position tensor, which reads the rows below the position and nothing else, so device mode keeps no key
    mask; a prefill attends its own unquantised keys / values and stores them with ``ops.kv8_append``.  The
    window step is not available on an fp8 cache.

    ``samples=n`` (default 1: the cache above, untouched): n continuations per prompt over ONE copy of the
    prompts' rows.  The states:
      * prefill — an ordinary host-mode pass over the G prompts (uniform or right-padded ragged) whose buffers
        ``prefix[layer]`` (G, max_len, 2, H, D) are read only from then on;
      * ``to_per_sequence(lens)`` fans out: ``prefix_len`` (G,) = lens, and the per-sequence triple (``_rows``,
        ``lens``, ``active``) gets B = G · n entries — row b is sample b % n of prompt b // n — with ``_rows`` = 0:
        the position in the row's own TAIL ``kv[layer]`` (B, tail_len, 2, H, D), the keys / values of the tokens
        the sample has generated;
      * from then on it is a per-sequence-mode cache whose positions are tail positions (``begin_step`` /
        ``end_step`` / ``active`` / ``snapshot`` / ``restore``; ``pos`` bounds them against ``tail_len``);
        ``embed`` reads wpe[prefix_len[b // n] + _rows[b]] and the attention layer calls ``step_shared``: one
        ``ops.attention_decode_prefix`` — the append to the tail and the attention over prefix, tail and new row.
    The window step and ``kv_dtype="fp8"`` are not available with ``samples > 1``."""

    def __init__(self, n_layer, max_len, kv_dtype=None, samples=1, tail_len=None):
        if kv_dtype not in (None, "fp8"):
            raise ValueError(f"kv_dtype must be None or 'fp8', got {kv_dtype!r}")
        if not isinstance(samples, int) or isinstance(samples, bool) or samples < 1:
            raise ValueError(f"samples must be an int >= 1, got {samples!r}")
        if samples > 1 and kv_dtype is not None:
            raise ValueError("a KV cache shared by several samples per prompt (samples > 1) has no fp8 form: kv_dtype "
                             "must be None")
        self.max_len, self.pos, self.mode = max_len, 0, "host"
        self.kv_dtype = kv_dtype
        self.samples = samples
        self.tail_len = max_len if tail_len is None else tail_len  # samples > 1: rows of each sample's own tail
        self.prefix = [None] * n_layer  # samples > 1: the prompts' rows (G, max_len, 2, H, D); kv holds the tails
        self.prefix_len = self._prefix_rows = None  # samples > 1: (G,) prompt lengths; the same per batch row (B,)
        self.kv = [None] * n_layer
        self.kv_scale = [None] * n_layer  # fp8 only
        self._host_pos = None  # fp8 only: the host position as a 1-element device tensor (eager steps)
        self._pos1 = self.mask = None  # device mode
        self._rows = self.lens = self.active = None  # per-sequence mode
        self.in_window = False  # inside ``windowed()``: the pass is the window step

    @contextlib.contextmanager
    def windowed(self):
        """The pass inside is the window step (``GPT2.decode_window``): ``embed`` reads T position rows
        per batch row and the attention layers call ``window`` instead of ``update`` / ``attend``."""
        self._need_per_seq("windowed")
        self._no_window()
        self.in_window = True
        try:
            yield self
        finally:
            self.in_window = False

    device_pos = property(lambda self: self.mode != "host")
    fp8 = property(lambda self: self.kv_dtype == "fp8")
    per_seq = property(lambda self: self.mode == "per_seq")
    shared = property(lambda self: self.samples > 1)  # several samples per prompt over one copy of its rows

    @property
    def pos_t(self):
        return self._rows if self.mode == "per_seq" else self._pos1 if self.mode == "device" else None

    def to_device_position(self):
        """Switch to device mode at the current host position."""
        if self._pos1 is None:
            dev = self.kv[0].device
            self._pos1 = torch.empty(1, dtype=torch.long, device=dev)
            if not self.fp8:  # the fp8 step reads rows < pos only: no key mask
                self.mask = torch.empty(1, 1, self.max_len, device=dev)
        self._pos1.fill_(self.pos)
        if self.mask is not None:
            self.mask.fill_(float("-inf"))
            self.mask[..., : self.pos] = 0.0
        self.mode = "device"

    def to_per_sequence(self, lens):
        """Switch to per-sequence mode after a right-padded prefill: row b holds ``lens[b]`` (B,)
        valid positions; what the prefill wrote at or past lens[b] is never read and is overwritten as
        the row grows.  The host ``pos`` becomes max(lens), which eager steps check against max_len."""
        lens = torch.as_tensor(lens, dtype=torch.long).reshape(-1)
        if self.shared:
            return self._fan_out(lens)
        self.pos = int(lens.max())
        lens = lens.to(self.kv[0].device)
        if self._rows is None or self._rows.shape != lens.shape:
            self._rows, self.lens, self.active = (torch.empty_like(lens) for _ in range(3))
        self._rows.copy_(lens)
        torch.add(lens, 1, out=self.lens)
        self.active.fill_(1)
        self.mode = "per_seq"

    def _fan_out(self, lens):
        """``to_per_sequence`` of a cache with ``samples`` = n > 1: the G prompts' rows become the read-only
        prefix and every prompt's n samples start their own tail at row 0.  The tails and the device tensors
        are allocated once (until the number of prompts changes): a captured step reads them by address."""
        pre, n = self.prefix[0], self.samples
        G, B = lens.numel(), lens.numel() * n
        if pre is None:
            raise ValueError("a shared KV cache fans out after a host-mode pass over the prompts (a prefill)")
        if pre.shape[0] != G:
            raise ValueError(f"the prefill wrote {pre.shape[0]} prompts, lens holds {G}")
        lens = lens.to(pre.device)
        if self.prefix_len is None or self.prefix_len.shape != lens.shape:
            self.prefix_len = torch.empty_like(lens)
            self._prefix_rows, self._rows, self.lens, self.active = (
                torch.empty(B, dtype=torch.long, device=pre.device) for _ in range(4))
            # zeroed like the prefix: rows at or past a position are never read, but should not look like data
            self.kv = [p.new_zeros(B, self.tail_len, *p.shape[2:]) for p in self.prefix]
        self.prefix_len.copy_(lens)
        self._prefix_rows.copy_(lens.repeat_interleave(n))
        self._rows.zero_()
        self.lens.fill_(1)
        self.active.fill_(1)
        self.pos, self.mode = 0, "per_seq"  # pos: the host bound of the TAIL positions from here on

    def reset(self):
        """Start a new sequence in the same buffers (host mode, position 0)."""
        self.pos, self.mode = 0, "host"

    def snapshot(self):
        """What a device-mode step changes, for ``restore`` (a warm-up or capture run of the step)."""
        return (self.pos, self._rows.clone(), self.lens.clone()) if self.mode == "per_seq" else (self.pos,)

    def restore(self, snap):
        """Undo the steps since ``snapshot``: the position(s); the rows they wrote are not valid yet."""
        self.pos = snap[0]
        if self.mode == "per_seq":
            self._rows.copy_(snap[1])
            self.lens.copy_(snap[2])
        else:
            self._pos1.fill_(self.pos)
            if self.mask is not None:
                self.mask[..., self.pos:] = float("-inf")

    def begin_step(self, T):
        """Before ``T`` tokens are embedded and appended: device mode opens the mask at the write row,
        the modes with a host position check the capacity."""
        if self.mode == "device":
            if self.mask is not None:
                self.mask.index_fill_(2, self._pos1, 0.0)
            elif T != 1:
                raise ValueError("an fp8 cache in device mode takes one token per step")
        elif self.mode == "per_seq" and T != 1:
            raise ValueError("a cache in per-sequence mode takes one token per row and step")
        elif self.shared and self.mode == "per_seq":
            if self.pos + T > self.tail_len:
                raise ValueError(f"KV cache full: {self.pos} + {T} tail rows > {self.tail_len}")
        elif self.pos + T > self.max_len:
            raise ValueError(f"KV cache full: {self.pos} + {T} > {self.max_len}")

    def end_step(self, T):
        """After the LM head: advance the position(s), once per step (device mode: one token)."""
        if self.mode == "device":
            self._pos1.add_(1)
            return
        if self.mode == "per_seq":
            self._rows.add_(self.active)
            self.lens.add_(self.active)
        self.pos += T

    # ---- the window step (per-sequence mode): T tokens per row, each row at its own position ----
    def _need_per_seq(self, what):
        if self.mode != "per_seq":
            raise ValueError(f"KVCache.{what} needs a cache in per-sequence mode (a ragged prefill)")

    def _no_window(self):
        if self.shared:
            raise ValueError("the window step is not available on a KV cache shared by several samples per prompt "
                             "(samples > 1)")

    def window(self, layer, qkv):
        """Append the key / value rows of ``qkv`` (B, T, 3, H, D) at each row's position and attend its T
        queries to the cached rows and the window so far: one ``ops.attention_window``.  The position
        does not move (``advance``): whatever the window wrote past it stays unread."""
        self._need_per_seq("window")
        self._no_window()
        if self.fp8:
            raise ValueError("the window step is not available on an fp8 KV cache")
        return ops.attention_window(qkv, self.kv[layer], self._rows)

    def advance(self, counts, bound=None):
        """Commit ``counts`` (B,) device integers of the rows a window step wrote: every active row moves
        by its own count.  No host value is read; ``bound`` (a host integer, if given) becomes ``pos``,
        the upper bound of the positions that eager steps check against max_len."""
        self._need_per_seq("advance")
        step = counts.to(self._rows.dtype) * self.active
        self._rows.add_(step)
        self.lens.add_(step)
        if bound is not None:
            self.pos = int(bound)

    def set_rows(self, rows, bound=None):
        """Put every row at position ``rows`` (B,) device integers — a draft cache following its target;
        rows at or past the new position are stale from then on.  ``bound``: as in ``advance``."""
        self._need_per_seq("set_rows")
        self._rows.copy_(rows)
        torch.add(self._rows, 1, out=self.lens)
        if bound is not None:
            self.pos = int(bound)

    def embed(self, idx, wte, wpe):
        """Token + position embedding of ``idx`` (B, T) at the cache position(s)."""
        if self.in_window:  # row b's tokens at wpe[pos_t[b] + i], the index clamped to the table
            self._need_per_seq("embed (window)")
            B, T = idx.shape
            at = (self._rows.view(B, 1) + torch.arange(T, device=idx.device)).clamp_(0, wpe.shape[0] - 1)
            return ops.embedding(idx.reshape(1, -1), wte, wpe.index_select(0, at.view(-1))).view(B, T, -1)
        if self.mode == "host":
            return ops.embedding(idx, wte, wpe[self.pos: self.pos + idx.shape[1]])
        if self.shared:  # a sample's position is its prompt's length plus its tail position, clamped to the table
            at = (self._prefix_rows + self._rows).clamp_(0, wpe.shape[0] - 1)
            return ops.embedding(idx.view(1, -1), wte, wpe.index_select(0, at)).view(idx.shape[0], 1, -1)
        rows = wpe.index_select(0, self.pos_t)
        if self.mode == "device":
            return ops.embedding(idx, wte, rows)
        # row b's position embedding is wpe[pos_t[b]]: the ids viewed as one sequence of B tokens
        return ops.embedding(idx.view(1, -1), wte, rows).view(idx.shape[0], 1, -1)

    def update(self, layer, kv):
        """Append ``kv`` (B, T, 2, H, D) — the key / value slice of the packed QKV projection — at
        the cache position; returns the (key, value) views the attention reads.  K and V share one
        buffer per layer, so an append is ONE copy (slice copy_ / index_copy_ / scatter_ by mode)."""
        store = self.prefix if self.shared else self.kv  # a shared cache's host-mode passes write the prompts' rows
        buf = store[layer]
        if self.mode == "host":
            B, T, _, H, D = kv.shape
            if buf is None:
                # zeroed, not empty: the device-mode step reads the WHOLE buffer under the key mask, and
                # a masked row still enters P·V as 0 · v — a NaN bit pattern in an unwritten row would
                # turn that into NaN
                buf = store[layer] = kv.new_zeros(B, self.max_len, 2, H, D)
            buf[:, self.pos: self.pos + T].copy_(kv)
            return buf[:, : self.pos + T, 0], buf[:, : self.pos + T, 1]
        if self.mode == "device":
            buf.index_copy_(1, self._pos1, kv)
        else:  # each row at its own position
            if kv.shape[1] != 1:
                raise ValueError("KV cache in per-sequence mode appends one token per step")
            buf.scatter_(1, self._rows.view(-1, 1, 1, 1, 1).expand_as(kv), kv)
        return buf[:, :, 0], buf[:, :, 1]

    def step_shared(self, layer, qkv):
        """The one-token step of a cache with ``samples > 1`` after the fan-out: ``qkv`` (B, 1, 3, H, D), the packed
        projection output -> (B, 1, H, D).  One ``ops.attention_decode_prefix``: row b's new key / value row is
        written to its tail at ``_rows[b]`` and its query attends its prompt's ``prefix_len[b // n]`` rows, its own
        tail rows below ``_rows[b]`` and the new row."""
        self._need_per_seq("step_shared")
        if qkv.shape[1] != 1:
            raise ValueError("a KV cache shared by several samples per prompt takes one token per row and step")
        return ops.attention_decode_prefix(qkv, self.prefix[layer], self.prefix_len, self.kv[layer], self._rows)

    def step8(self, layer, qkv, causal):
        """An fp8 cache's append and attention in one: ``qkv`` (B, T, 3, H, D), the packed projection output,
        -> (B, T, H, D).  T == 1 (every mode): ``ops.attention_decode_kv8`` at the mode's position tensor.  A
        host-mode prefill at position 0 attends its own unquantised keys / values, then ``ops.kv8_append`` stores
        the T rows (a ragged one writes junk past lens[b] as the bf16 cache does; it is never read).  T > 1 at a
        position > 0 (host mode) is the slow composed path: the rows below the position dequantised, this pass's
        own rows after them, the causal attention, then the append."""
        B, T, _, H, D = qkv.shape
        if self.kv[layer] is None:
            if self.mode != "host":
                raise ValueError("an fp8 KV cache is allocated by a host-mode pass (a prefill)")
            # rows at or past a position are never read, but a fresh buffer should not look like data
            self.kv[layer] = torch.zeros(B, self.max_len, 2, H, D, dtype=torch.uint8, device=qkv.device)
            self.kv_scale[layer] = torch.ones(B, self.max_len, 2, H, dtype=torch.float32, device=qkv.device)
        kv8, sc = self.kv[layer], self.kv_scale[layer]
        if self.mode == "host":
            if self._host_pos is None:
                self._host_pos = torch.empty(1, dtype=torch.long, device=qkv.device)
            pos = self._host_pos.fill_(self.pos)  # host mode is eager only
        else:
            pos = self.pos_t
        if T == 1:
            return ops.attention_decode_kv8(qkv, kv8, sc, pos)
        if self.mode != "host":
            raise ValueError("an fp8 KV cache takes several tokens per step in host mode only")
        q, k, v = qkv.unbind(2)
        if self.pos > 0:
            old = ops.kv8_dequantize(kv8[:, : self.pos], sc[:, : self.pos]).to(qkv.dtype)
            k, v = torch.cat([old[:, :, 0], k], 1), torch.cat([old[:, :, 1], v], 1)
        a = ops.attention(q, k, v, causal=causal)
        ops.kv8_append(qkv[:, :, 1:3], kv8, sc, pos)
        return a

    def attend(self, q, k, v, causal):
        """Attention of this step's queries (B, T, H, D) over the key / value views of the append."""
        if self.mode == "per_seq":  # each row reads its own lens[b] keys
            return ops.attention_decode(q, k, v, lens=self.lens)
        if self.mode == "device":  # the key mask carries causality
            return ops.attention_decode(q, k, v, self.mask) if q.shape[1] == 1 else ops.attention(q, k, v, bias=self.mask)
        return ops.attention(q, k, v, causal=causal)


def host_lens(name, lens, B, T):
    """``lens`` (tensor or sequence) as B host integers in [1, T]."""
    lens = [int(n) for n in (lens.tolist() if torch.is_tensor(lens) else lens)]
    if len(lens) != B or min(lens) < 1 or max(lens) > T:
        raise ValueError(f"{name} must hold {B} values in [1, {T}], got {lens}")
    return lens


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


# captured decode steps kept per model (least recently used evicted first): each holds a KV cache of
# 2 · n_layer · B · length · n_embd elements (≈ 2.4 GB for GPT-2-small at B = 64, length 1024; ≈ 1.3 GB with
# kv_dtype="fp8": a byte per element and 4 bytes of scale per 64)
DECODE_GRAPHS_MAX = int(os.environ.get("REPLICANN_DECODE_GRAPHS", "4"))
DECODE_LEN_BUCKET = 64  # cache lengths are rounded up to this (capped at block_size): one graph per bucket
DECODE_EOS_CHECK = 8  # ragged generate: "has every row finished?" is asked of the device every this many steps


class _GraphRegistry(dict):
    """One model's captured decode steps kept across ``generate`` calls, least recently used first:
    (batch, cache length, dtype, device, parameter storage[, "ragged" for the per-sequence step]
    [, "sampler" for a step captured together with the native sampler][, "window", T for the window step of
    T tokens per row: its output is the greedy ids (B, T)][, "logits" for the window step whose output is the
    logits (B, T, vocab) instead][, "fp8" for a step over an fp8 KV cache, always last][, "prompts", G, "tail", tail length, "samples", n for the
    step of n samples per prompt over a shared prompt cache, always last: batch is then G · n and cache length the
    prompts' bucket, so the key holds everything its buffers' shapes depend on and a shared step never aliases a
    plain one]) → (cache, graph, token buffer, logits), so a serving loop captures once per (batch, length bucket).  A sampler entry holds the
    sampled tokens (B, 1) in place of the logits, then the device tensor its settings are read from:
    one graph whatever the temperature / top_k / top_p.
    At most DECODE_GRAPHS_MAX (REPLICANN_DECODE_GRAPHS, default 4) are kept; each holds its KV cache."""

    def lookup(self, model, B, L, ragged, use, sampler=False, window=None, logits=False, kv_dtype=None, shared=None):
        """(key, its stored entry — now the most recently used — or None).  The parameters' storage
        is part of the key: a graph reads them by address, so entries captured before a parameter was
        re-assigned (p.data = ...) are dropped here, whether or not this call will ``use`` a graph."""
        sig = tuple(p.data_ptr() for p in model.parameters())
        key = (B, L, model.wte.dtype, model.wte.device, sig) + (("ragged",) if ragged else ())
        key += ("sampler",) if sampler else ()
        key += ("window", window) if window else ()  # the captured window step of this many tokens per row
        key += ("logits",) if logits else ()  # ... returning its logits, not the greedy ids
        key += (kv_dtype,) if kv_dtype else ()  # an fp8 cache's step never aliases the bf16 one
        # shared = (tail length, n): n samples per prompt over one copy of the B // n prompts' rows
        key += ("prompts", B // shared[1], "tail", shared[0], "samples", shared[1]) if shared else ()
        for k in [k for k in self if k[4] != sig]:
            del self[k]
        entry = self.pop(key, None) if use else None
        if entry is not None:
            self[key] = entry
        return key, entry

    def make_room(self):
        while len(self) >= max(DECODE_GRAPHS_MAX, 1):
            self.pop(next(iter(self)))


# kept outside the module's attributes (weak-keyed), so copying / pickling a model never touches graph objects
_REGISTRIES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def registry(model):
    return _REGISTRIES.setdefault(model, _GraphRegistry())


def sampler_params(temperature, top_k, top_p, device=None):
    """(temperature, top_k, top_p) as the 3 fp32 values ``ops.sample_logits(params=...)`` reads (0 / 1: filter off)."""
    return torch.tensor([temperature, top_k or 0, 1.0 if top_p is None else top_p], dtype=torch.float32, device=device)


def _sampled_step(model, tok, cache, params):
    """The one-token step followed by the native sampler on a fresh device seed: (B, 1) token ids."""
    logits = model._device_position_step(tok, cache)
    return ops.sample_logits(logits, params=params, seed_buf=rng.next_seed(logits.device))[0]


def capture_step(model, cache, B, sampler=None):
    """Record the one-token decode step as a hipGraph (after one eager warm-up that tunes the
    decode GEMM shapes); the caller writes the next token into ``tok`` and replays.

    ``sampler`` (host (temperature, top_k, top_p) to start from): the step and the native sampler are
    recorded together — after the LM head the graph draws a device seed (``ops.rng``) and samples into
    a static (B, 1) token buffer, its settings read from a device tensor; returns (graph, tok, tokens,
    params).  The ``ops.rng`` states are restored around the warm-up and the capture: capturing
    consumes no draws, so a capturing call and a replaying one started from the same state agree."""
    dev = model.wte.device
    tok = torch.zeros(B, 1, dtype=torch.long, device=dev)
    if not cache.device_pos:  # uniform: the prefill ran in host mode (ragged: it left per-sequence mode)
        cache.to_device_position()
    params = None if sampler is None else sampler_params(*sampler, device=dev)
    step = model._device_position_step if sampler is None else (lambda t, c: _sampled_step(model, t, c, params))
    seeds = [(st, st.clone()) for st in rng.state_tensors(dev if sampler is not None else None)]

    def restore():
        cache.restore(snap)
        for st, saved in seeds:
            st.copy_(saved)

    snap = cache.snapshot()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step(tok, cache)
    torch.cuda.current_stream(dev).wait_stream(side)
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(tok, cache)
    restore()
    return (graph, tok, out) if sampler is None else (graph, tok, out, params)


def capture_window(model, cache, B, T, logits=False):
    """Record the window step ``model.decode_window`` of ``T`` tokens per row as a hipGraph, the way
    ``capture_step`` does (one eager warm-up on a side stream; ``cache`` — in per-sequence mode — is
    put back after both runs, so the positions after the capture equal the positions before it; the
    rows the runs wrote are past them: not valid).  Returns (graph, tok (B, T), ids (B, T)): the caller
    writes the window's tokens into ``tok``, replays and reads the greedy ids — with ``logits`` the step is
    ``model.decode_window_logits`` and the static output its logits (B, T, vocab)."""
    step = model.decode_window_logits if logits else model.decode_window
    dev = model.wte.device
    tok = torch.zeros(B, T, dtype=torch.long, device=dev)
    snap = cache.snapshot()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step(tok, cache)
    torch.cuda.current_stream(dev).wait_stream(side)
    cache.restore(snap)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(tok, cache)
    cache.restore(snap)
    return graph, tok, out


def accept(drafts, greedy, *, matched=None, budget=None, finished=None, eos=None, pad=0):
    """What one round of speculative decoding commits — a pure tensor function, no host value.

    ``drafts`` (B, K): the draft model's tokens d_1 .. d_K after the pending token; ``greedy``
    (B, K+1): the target's greedy token after each window position [pending, d_1 .. d_K].  With ``a``
    the length of the prefix on which they agree (d_j == greedy[j-1] for j <= a), a row commits
    d_1 .. d_a and the target's own token greedy[a]: the a + 1 tokens greedy[:a+1].  They are cut after
    the first ``eos`` (kept) and at the row's ``budget`` (B,), the tokens it may still emit; a
    ``finished`` (B,) row commits nothing.

    Speculative sampling passes what ``ops.speculative_verify`` returned: ``greedy`` is then its tokens (B, K+1)
    — the accepted drafts and the resampled / bonus token — and ``matched`` (B,) its accepted length a, which
    the verifier decided; the cuts are the same.

    Returns (count (B,), tokens (B, K+1), matched (B,)): how many tokens each row commits, the tokens
    themselves (``pad`` past count) and the agreed length a before any cut."""
    B, K = drafts.shape
    j = torch.arange(K + 1, device=drafts.device).view(1, K + 1)
    if matched is None:
        matched = (drafts == greedy[:, :K]).long().cumprod(1).sum(1)
    count = matched + 1
    if eos is not None:  # the first EOS among the committed tokens ends them
        first = torch.where(greedy == eos, j, K + 1).amin(1)
        count = torch.minimum(count, first + 1)
    if budget is not None:
        count = torch.minimum(count, budget.clamp(min=0))
    if finished is not None:
        count = count.masked_fill(finished, 0)
    return count, torch.where(j < count.view(B, 1), greedy, torch.full_like(greedy, pad)), matched


def _check_draft(model, draft, draft_k, temperature, need, native):
    if temperature != 0 and not native:
        raise ValueError("generate(draft=...) with sampler='torch' is greedy: temperature must be 0 (speculative "
                         "sampling, temperature > 0 with a draft model, needs sampler='native')")
    if not isinstance(draft_k, int) or not 1 <= draft_k <= 15:
        raise ValueError(f"draft_k must be in 1..15, got {draft_k}")
    for what, a, b in (("vocab_size", model.config.vocab_size, draft.config.vocab_size),
                       ("device", model.wte.device, draft.wte.device), ("dtype", model.wte.dtype, draft.wte.dtype)):
        if a != b:
            raise ValueError(f"the draft model's {what} ({b}) differs from the target's ({a})")
    for name, m in (("target", model), ("draft", draft)):
        # the window writes draft_k rows past the last committed one, and wpe has no rows beyond block_size
        if need + draft_k > m.config.block_size:
            raise ValueError(f"prompt + new tokens + draft_k = {need + draft_k} exceeds the {name} model's block_size "
                             f"{m.config.block_size}")


class _WindowDriver:
    """One speculative ``generate`` call's target side: the cache and the window step of T tokens per
    row, eager or as a hipGraph kept in the model's registry under (..., "ragged", "window", T).  ``logits``: the
    step returns the window's logits (B, T, vocab), not the greedy ids (its own registry key)."""

    def __init__(self, model, B, length, T, graph, logits=False):
        length = min(model.config.block_size, -(-length // DECODE_LEN_BUCKET) * DECODE_LEN_BUCKET)
        self.model, self.B, self.T, self.graph, self.graphs = model, B, T, graph, registry(model)
        self.logits = logits
        self.key, self.entry = self.graphs.lookup(model, B, length, True, graph, window=T, logits=logits)
        self.cache = KVCache(model.config.n_layer, length) if self.entry is None else self.entry[0]
        self.cache.reset()

    def step(self, toks):
        """Greedy ids (B, T) — or logits (B, T, vocab) — after every position of the window ``toks`` (B, T); a
        replay returns its static buffer."""
        if not self.graph:
            return (self.model.decode_window_logits if self.logits else self.model.decode_window)(toks, self.cache)
        if self.entry is None:
            self.graphs.make_room()  # before the capture allocates
            self.entry = self.graphs[self.key] = (self.cache, *capture_window(self.model, self.cache, self.B, self.T,
                                                                              self.logits))
        _, graph, buf, out = self.entry
        buf.copy_(toks)
        graph.replay()
        return out


def _speculative_loop(model, draft, idx, plens, max_new_tokens, K, eos, pad, use_graph, ragged, stats, sampling=None):
    """Generation of ``model`` with ``draft`` proposing K tokens a round (see ``generate``): greedy, or with
    ``sampling`` = (temperature, top_k, top_p, generator) speculative sampling on the native sampler."""
    (B, Tm), dev = idx.shape, idx.device  # idx: the prompts cut to the longest one
    V = model.config.vocab_size

    def pick(logits):
        """(B, V) logits → (B,) ids: the argmax, or ``ops.sample_logits`` under the call's settings (a device
        seed on a GPU model, the host generator's uniforms on a CPU model)."""
        if sampling is None:
            return logits.argmax(-1)
        t, k, p, gen = sampling
        if logits.is_cuda:
            return ops.sample_logits(logits, t, k, p, seed_buf=rng.next_seed(dev))[0][:, 0]
        return ops.sample_logits(logits.float(), t, k, p, u=torch.rand(B, generator=gen))[0][:, 0]

    if pad is None:
        pad = eos if eos is not None else 0
    need = Tm + max_new_tokens + K
    target = _WindowDriver(model, B, need, K + 1, use_graph, logits=sampling is not None)
    drafter = _StepDriver(draft, B, need, True, use_graph, (0, None, None, None), False)
    lens = torch.tensor(plens, dtype=torch.long, device=dev)  # each row's length so far
    # rows prompt ‖ generated, pad elsewhere (K + 1 spare columns: a round's padded tail lands in range)
    tokens = torch.full((B, need + 1), pad, dtype=torch.long, device=dev)
    keep = torch.arange(Tm, device=dev).unsqueeze(0) < lens.unsqueeze(1)
    tokens[:, :Tm] = torch.where(keep, idx, tokens[:, :Tm])
    j = torch.arange(K + 1, device=dev).view(1, K + 1)
    # both models prefill the prompts; the target's first token is committed at once and is "pending": the
    # last committed token, not yet in either cache (it goes to row cache.pos_t of both)
    pending = pick(model.decode_step(idx, target.cache, lens=plens))
    draft.decode_step(idx, drafter.cache, lens=plens)
    tokens.scatter_(1, lens.view(B, 1), pending.view(B, 1))
    lens += 1
    budget = torch.full((B,), max_new_tokens - 1, dtype=torch.long, device=dev)
    finished = budget <= 0
    if eos is not None:
        finished |= pending == eos
    drafted, accepted = torch.zeros_like(lens), torch.zeros_like(lens)
    rounds_run = torch.zeros((), dtype=torch.long, device=dev)
    drafts = torch.empty(B, K, dtype=torch.long, device=dev)
    if sampling is not None:
        # the rows the drafts are drawn from: a replayed step's static logits are overwritten by the next replay.
        # Rows padded to 16 bytes, like the target's (a slice of the padded LM head): the verifier reads both in
        # one slot mapping with vector loads
        dlogits = torch.empty(B, K, -(-V // 8) * 8, dtype=torch.float32 if not model.wte.is_cuda else model.wte.dtype,
                              device=dev)[..., :V]
    # an unfinished row commits 1 .. K + 1 tokens a round: no row can be done before `least` rounds without an
    # EOS, and every row is after `most`; in between the device is asked every DECODE_EOS_CHECK rounds
    most, least = max_new_tokens - 1, -(-(max_new_tokens - 1) // (K + 1))
    for r in range(most):
        ask = (r % DECODE_EOS_CHECK == 0) if eos is not None else (r >= least and (r - least) % DECODE_EOS_CHECK == 0)
        if r and ask and bool(finished.all()):
            break  # the one host sync of the stop logic
        # the host bound of every row's position in this round: pending's row, then up to K drafted rows
        top = min(Tm + r * (K + 1), Tm + max_new_tokens - 1)
        live = ~finished
        drafter.cache.active.copy_(live)  # finished rows stay where they are
        drafter.cache.pos = top
        tok = pending.view(B, 1)
        # K + 1 draft steps: the last one only writes d_K's cache row (needed when every draft is accepted)
        for i in range(K + 1):
            logits = drafter.step(tok)
            if i < K:
                tok = pick(logits).view(B, 1)
                drafts[:, i] = tok[:, 0]
                if sampling is not None:
                    dlogits[:, i].copy_(logits)
        greedy = target.step(torch.cat([pending.view(B, 1), drafts], 1))
        matched = None
        if sampling is not None:  # `greedy` holds the window's logits: the verifier's tokens take its place
            t, k, p, gen = sampling
            if greedy.is_cuda:  # two launches after the window step (or its replay); no host value
                greedy, matched = ops.speculative_verify(greedy, dlogits, drafts, t, k, p, seed_buf=rng.next_seed(dev),
                                                         check_drafts=False)
            else:
                greedy, matched = ops.speculative_verify(greedy.float(), dlogits, drafts, t, k, p,
                                                         u=torch.rand(B, K + 1, 2, generator=gen))
        count, out, matched = accept(drafts, greedy, matched=matched, budget=budget, finished=finished, eos=eos, pad=pad)
        tokens.scatter_(1, lens.view(B, 1) + j, out)  # pad past count: those columns are not committed yet
        pending = torch.where(count > 0, out.gather(1, (count - 1).clamp(min=0).view(B, 1))[:, 0], pending)
        lens += count
        budget -= count
        drafted += K * live
        accepted += matched * live
        rounds_run += live.any()
        finished = finished | (budget <= 0)
        if eos is not None:
            finished |= ((out == eos) & (j < count.view(B, 1))).any(1)
        target.cache.advance(count, bound=min(top + K + 1, Tm + max_new_tokens))
        drafter.cache.set_rows(target.cache.pos_t)
    if stats is not None:
        stats.update(rounds=int(rounds_run), drafted=drafted.clone(), accepted=accepted.clone())
    if ragged:
        return tokens[:, : int(lens.max())], lens
    return tokens[:, : Tm + max_new_tokens]


class _StepDriver:
    """One ``generate`` call's cache and one-token step.  With ``graph``, an earlier call's cache and
    captured step of the same key are reused; failing that the first ``step`` captures (and stores) one."""

    def __init__(self, model, B, length, ragged, graph, sampling, native, kv_dtype=None, samples=1, new=None):
        c = model.config

        def bucket(x):
            return min(c.block_size, -(-x // DECODE_LEN_BUCKET) * DECODE_LEN_BUCKET)

        shared = None
        if samples > 1:  # B = G · samples rows; length: the longest prompt; new: the new-token budget (the tails)
            length, shared = bucket(length), (bucket(new), samples)
        elif graph or ragged:  # one captured step (and cache) serves every length of a bucket
            length = bucket(length)
        self.model, self.B, self.graph, self.graphs = model, B, graph, registry(model)
        # sampling: (temperature, top_k, generator, top_p); native: ops.sample_logits instead of _sample
        self.sampling, self.native = sampling, native
        self.fused = native and graph  # the sampler is part of the captured step
        self.settings_sent = False  # fused: has this call written its settings into the graph's tensor?
        self.key, self.entry = self.graphs.lookup(model, B, length, ragged, graph, sampler=self.fused,
                                                  kv_dtype=kv_dtype, shared=shared)
        if self.entry is not None:
            self.cache = self.entry[0]
        elif shared:
            self.cache = KVCache(c.n_layer, length, samples=samples, tail_len=shared[0])
        else:
            self.cache = KVCache(c.n_layer, length, kv_dtype)
        self.cache.reset()

    def step(self, tok):
        """Logits (B, vocab) after appending ``tok`` (B, 1); a replay returns its static buffer (of a
        step captured with the sampler: the sampled tokens (B, 1))."""
        if not self.graph:
            return self.model._device_position_step(tok, self.cache)
        if self.entry is None:
            self.graphs.make_room()  # before the capture allocates
            t, k, _, p = self.sampling
            captured = self.model._capture_decode(self.cache, self.B, *([(t, k, p)] if self.fused else []))
            self.entry = self.graphs[self.key] = (self.cache, *captured)
            self.settings_sent = True  # a new sampler entry starts from this call's settings
        elif not self.cache.device_pos:  # a reused uniform cache: its prefill ran in host mode
            self.cache.to_device_position()
        _, graph, buf, out = self.entry[:4]
        if self.fused and not self.settings_sent:  # a stored graph: this call's settings, once
            t, k, _, p = self.sampling
            self.entry[4].copy_(sampler_params(t, k, p))
            self.settings_sent = True
        buf.copy_(tok)
        graph.replay()
        return out

    def pick(self, logits):
        """(B, vocab) logits → (B, 1) token ids by this call's sampler; what a step captured with the
        sampler returned is the tokens already: a copy (the next replay rewrites that static buffer)."""
        if logits.dtype == torch.long:
            return logits.clone()
        temperature, top_k, generator, top_p = self.sampling
        if not self.native:
            return _sample(logits.float(), *self.sampling)
        if not logits.is_cuda:  # the reference math of ops.sample_logits on uniforms from the host generator
            u = torch.rand(logits.shape[0], generator=generator)
            return ops.sample_logits(logits.float(), temperature, top_k, top_p, u=u)[0]
        return ops.sample_logits(logits, temperature, top_k, top_p, seed_buf=rng.next_seed(logits.device))[0]


@torch.no_grad()
def generate(model, idx, max_new_tokens, *, temperature=1.0, top_k=None, top_p=None, generator=None, graph=None,
             prompt_lens=None, eos_token_id=None, pad_token_id=None, sampler="torch", draft=None, draft_k=4,
             stats=None, kv_dtype=None, num_samples=1):
    """Autoregressive sampling with a KV cache: ``idx`` (B, T0) prompt → (B, T0 + max_new_tokens).
    ``temperature`` 0 = greedy; ``top_k`` / ``top_p`` restrict sampling.  One prefill pass over the prompt, then one-token steps whose
    attention reads the cached keys / values (no recomputation of the prefix).  ``graph``
    (default: on for GPU models): the one-token step is captured once as a hipGraph and replayed
    (per-step values live on the device), so a step costs its kernels, not ~130 host launches.

    ``sampler``: ``"torch"`` (default) samples with ATen ops on the host's ``generator`` after every
    step; ``"native"`` with the fused ``ops.sample_logits`` kernel (its semantics differ only inside
    tie groups: whole groups are kept).  On a GPU model its randomness is the device seed stream of
    ``ops.rng`` (``ops.rng.manual_seed``; a ``generator`` is an error) and, with ``graph``, the sampler
    is captured with the step: a generation is a prefill, one sample and replays.  On a CPU model the
    uniforms come from ``generator``.

    Ragged batches / stopping (either of ``prompt_lens``, ``eos_token_id`` given): ``idx`` is
    right-padded, row b's prompt is ``idx[b, :prompt_lens[b]]`` (default: all of it) and whatever the
    padding holds is ignored.  A row is finished once it has emitted ``eos_token_id`` (kept in the
    output); from then on it emits ``pad_token_id`` (default: the EOS id, else 0) and its position
    stops.  Generation ends early once every row is finished (asked of the device every
    DECODE_EOS_CHECK steps).  Returns ``(tokens, lens)``: tokens (B, max(lens)), rows
    ``prompt_b ‖ generated_b`` right-padded with the pad id, and lens (B,) each row's total length.

    Speculative decoding (``draft``: a smaller model of the same vocabulary, device and dtype).  With
    ``temperature=0`` the output is this model's greedy generation, token for token up to near-ties of
    the arithmetic, produced in rounds.  Both models prefill the prompts; a round replays the draft's
    one-token step ``draft_k`` + 1 times from the last committed token (the extra step writes the last
    draft's cache row; its output is dropped), runs this model's window step over the committed token
    and the ``draft_k`` drafts (``decode_window``: one pass of about one step's cost), commits what
    ``accept`` keeps — the agreed drafts plus one token of this model's own, cut at an EOS and at
    ``max_new_tokens`` — and moves both caches to the committed position, all on the device.  The
    return types are the same; ``stats`` (a dict) receives ``rounds`` and, per row, ``drafted`` and
    ``accepted`` (draft tokens proposed / agreed with).  With ``temperature > 0`` it is speculative sampling
    and needs ``sampler="native"`` (the default sampler raises): the first token and every draft token are drawn
    with ``ops.sample_logits`` under the call's ``temperature`` / ``top_k`` / ``top_p``, the draft logits of a
    round are kept, the window step returns this model's logits (``decode_window_logits``) and
    ``ops.speculative_verify`` accepts each draft with probability min(1, p/q) and draws the token after the
    last accepted one from the residual max(p - q, 0) (after ``draft_k`` accepted drafts: a bonus token from
    p), so every committed token is distributed as this model's own sampling; ``accept`` applies the same
    cuts.  The verifier's two launches are issued after the window step (with ``graph``: after its replay, not
    captured with it); the randomness is that of ``sampler="native"``.  The caches hold ``draft_k`` rows more than the
    tokens: prompt + ``max_new_tokens`` + ``draft_k`` must fit both models' block_size.

    ``kv_dtype="fp8"`` (default None: the cache in the model's dtype): the KV cache is kept as OCP e4m3 bytes
    with one power-of-two scale per 64-element head row (``decoding.KVCache``, ``ops.kv8``) — 0.53 of the
    bytes, in memory and per step — and the one-token step's attention quantises and appends the new row
    itself (``ops.attention_decode_kv8``).  The prefill attends its own unquantised keys / values.  Every mode
    above works with it except ``draft``, which raises: the window step has no fp8 form.

    ``num_samples=n`` (default 1: everything above, unchanged): n continuations of every prompt — ``idx`` is
    (G, T0) and the result has G · n rows, row g · n + s being sample s of prompt g (with ``prompt_lens`` /
    ``eos_token_id``: ``(tokens, lens)`` over G · n rows).  The prompts are prefilled ONCE, at batch G; the last
    position's logits are repeated n times and every sample draws its own first token with the call's sampler;
    the one-token steps then run at batch G · n over a cache that keeps one copy of each prompt's rows and a
    short tail per sample (``decoding.KVCache(samples=n)``, ``ops.attention_decode_prefix``): the prompt's keys /
    values are stored once and read once per step, not n times.  Uniform or ragged prompts, EOS (rows finish
    independently), eager or captured steps and both samplers work with it; ``draft`` and ``kv_dtype`` raise."""
    if not isinstance(num_samples, int) or isinstance(num_samples, bool) or num_samples < 1:
        raise ValueError(f"num_samples must be an int >= 1, got {num_samples!r}")
    if num_samples > 1 and draft is not None:
        raise ValueError("generate(num_samples > 1) with draft= is not supported: speculative decoding over a shared "
                         "prompt cache needs a window step it does not have")
    if num_samples > 1 and kv_dtype is not None:
        raise ValueError("generate(num_samples > 1) with kv_dtype= is not supported: the shared prompt cache has no "
                         "fp8 form")
    B, T0 = idx.shape
    ragged = prompt_lens is not None or eos_token_id is not None
    if top_p is not None and not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must be in (0, 1], got {top_p}")
    if sampler not in ("torch", "native"):
        raise ValueError(f"sampler must be 'torch' or 'native', got {sampler!r}")
    if kv_dtype not in (None, "fp8"):
        raise ValueError(f"kv_dtype must be None or 'fp8', got {kv_dtype!r}")
    if draft is not None and kv_dtype is not None:
        raise ValueError("generate(draft=...) needs the window step, which an fp8 KV cache does not have: "
                         "kv_dtype must be None")
    native = sampler == "native"
    if native and generator is not None and model.wte.is_cuda:
        raise ValueError("sampler='native' on a GPU model draws from the device seed stream "
                         "(ops.rng.manual_seed), not from a torch.Generator")
    if native and (temperature < 0 or (top_k is not None and top_k < 0)):
        raise ValueError(f"sampler='native' needs temperature >= 0 and top_k >= 0, got {temperature}, {top_k}")
    plens = [T0] * B if prompt_lens is None else host_lens("prompt_lens", prompt_lens, B, T0)
    Tm = max(plens)
    if (ragged or num_samples > 1) and max_new_tokens < 1:
        raise ValueError(f"max_new_tokens must be at least 1, got {max_new_tokens}")
    if Tm + max_new_tokens > model.config.block_size:
        raise ValueError(f"prompt {Tm} + {max_new_tokens} new tokens exceeds block_size {model.config.block_size}")
    use_graph = (model.wte.is_cuda if graph is None else graph) and max_new_tokens > 2
    if draft is not None:
        if max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be at least 1, got {max_new_tokens}")
        _check_draft(model, draft, draft_k, temperature, Tm + max_new_tokens, native)
        modes = [(m, m.training) for m in (model, draft)]
        try:
            for m, _ in modes:
                m.eval()
            return _speculative_loop(model, draft, idx[:, :Tm], plens, max_new_tokens, draft_k, eos_token_id,
                                     pad_token_id, use_graph, ragged, stats,
                                     (temperature, top_k, top_p, generator) if temperature != 0 else None)
        finally:
            for m, was in modes:
                m.train(was)
    was_training = model.training
    model.eval()
    try:
        if num_samples > 1:  # one prefill at batch B, then the ragged loop over B · num_samples rows
            driver = _StepDriver(model, B * num_samples, Tm, True, use_graph, (temperature, top_k, generator, top_p),
                                 native, samples=num_samples, new=max_new_tokens)
            out = _ragged_loop(driver, idx[:, :Tm], plens, max_new_tokens, eos_token_id, pad_token_id, num_samples)
            return out if ragged else out[0]  # no EOS, equal lengths: every row is full
        driver = _StepDriver(model, B, Tm + max_new_tokens, ragged, use_graph,
                             (temperature, top_k, generator, top_p), native, kv_dtype)
        if ragged:
            return _ragged_loop(driver, idx[:, :Tm], plens, max_new_tokens, eos_token_id, pad_token_id)
        logits = model.decode_step(idx, driver.cache)
        out = [idx]
        for i in range(max_new_tokens):
            out.append(driver.pick(logits))
            if i + 1 < max_new_tokens:
                logits = driver.step(out[-1])
        return torch.cat(out, 1)
    finally:
        model.train(was_training)


def _ragged_loop(driver, idx, plens, max_new_tokens, eos, pad, samples=1):
    logits = driver.model.decode_step(idx, driver.cache, lens=plens)
    if samples > 1:  # the one prefill serves every sample of a prompt: each draws its own first token
        idx, logits = idx.repeat_interleave(samples, 0), logits.repeat_interleave(samples, 0)
        plens = [n for n in plens for _ in range(samples)]
    (B, Tm), dev = idx.shape, idx.device  # idx: the prompts cut to the longest one
    if pad is None:
        pad = eos if eos is not None else 0
    lens = torch.tensor(plens, dtype=torch.long, device=dev)  # each row's length so far
    # rows prompt ‖ generated, pad elsewhere (one spare column: a finished row's write lands in range)
    tokens = torch.full((B, Tm + max_new_tokens + 1), pad, dtype=torch.long, device=dev)
    keep = torch.arange(Tm, device=dev).unsqueeze(0) < lens.unsqueeze(1)
    tokens[:, :Tm] = torch.where(keep, idx, tokens[:, :Tm])
    finished = torch.zeros(B, dtype=torch.bool, device=dev)
    for i in range(max_new_tokens):
        nxt = driver.pick(logits)
        nxt = torch.where(finished.unsqueeze(1), torch.full_like(nxt, pad), nxt)  # finished rows emit pad
        tokens.scatter_(1, lens.unsqueeze(1), nxt)
        lens += ~finished
        if eos is not None:
            finished |= nxt.squeeze(1) == eos
        if i + 1 == max_new_tokens:
            break
        if eos is not None and (i + 1) % DECODE_EOS_CHECK == 0 and bool(finished.all()):
            break  # the one host sync of the stop logic
        driver.cache.active.copy_(~finished)  # finished rows stay where they are
        logits = driver.step(nxt)
    return tokens[:, : int(lens.max())], lens


def generate_batch(model, prompts, max_new_tokens, **kw):
    """``generate`` for a list of 1-D token tensors of any lengths: pads them, runs the ragged
    path and returns a list of 1-D tensors ``prompt_b ‖ generated_b``, each trimmed to its length.
    With ``num_samples=n`` the list holds n tensors per prompt, prompt by prompt."""
    plens = [int(p.numel()) for p in prompts]
    if not plens or min(plens) < 1:
        raise ValueError("generate_batch needs at least one prompt, each of at least one token")
    idx = torch.zeros(len(prompts), max(plens), dtype=torch.long, device=model.wte.device)
    for b, p in enumerate(prompts):
        idx[b, : plens[b]] = p.to(idx.device)
    tokens, lens = model.generate(idx, max_new_tokens, prompt_lens=plens, **kw)
    return [tokens[b, :n] for b, n in enumerate(lens.tolist())]
