"""Linear layers on the gfx950 MFMA GEMM (csrc/kernels/gemm_bf16.hip).

Replaces the reference's per-head ``nn.Linear`` launches
(reference ``src/replicann/nn/attention.py:135-137``, ``arch/transformer.py:29-31``)
with one GEMM per projection whose epilogue fuses bias, activation
(ReLU / tanh-GELU), residual add and bf16 down-cast.

Backward = one dgrad GEMM (dX = dH·W, "NN") + one wgrad GEMM
(dW = dHᵀ·X, "TN", split-K over the token dimension) + a fused
activation-backward / bias-gradient reduction kernel.  All three GEMM layouts
run on the same kernel: K-contiguous operands are read from LDS with
``ds_read_b128``, M/N-contiguous ones with the ``ds_read_b64_tr_b16``
hardware transpose, so no operand is ever transposed in HBM.

CPU tensors take the plain ATen path (same math, fp32 accumulation).
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .. import _ext

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
# GEMM-epilogue-only codes: 5 = GELU whose pre-activation buffer receives gelu'(h) instead of h;
# 6 = its fused backward, out = (A·B) ⊙ pre (one multiply; see csrc/include/common.h)
ACT_GELU_D, ACT_MUL_BWD = 5, 6
_ACTS = {None: ACT_NONE, "none": ACT_NONE, "relu": ACT_RELU, "gelu": ACT_GELU}


def _act_ref(h: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return F.relu(h)
    if act in (ACT_GELU, ACT_GELU_D):
        return F.gelu(h, approximate="tanh")
    return h


def _pre_ref(h: torch.Tensor, act: int) -> torch.Tensor:
    """What the forward epilogue writes into the pre-activation buffer."""
    if act == ACT_GELU_D:
        return _act_grad_ref(torch.ones_like(h), h, ACT_GELU)
    return h


def _act_grad_ref(dy: torch.Tensor, h: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_RELU:
        return dy * (h > 0).to(dy.dtype)
    if act == ACT_GELU:
        hf = h.float()
        c = math.sqrt(2.0 / math.pi)
        u = c * (hf + 0.044715 * hf**3)
        t = torch.tanh(u)
        d = 0.5 * (1 + t) + 0.5 * hf * (1 - t * t) * c * (1 + 3 * 0.044715 * hf * hf)
        return (dy.float() * d).to(dy.dtype)
    return dy


# --------------------------------------------------------------------------
# raw GEMM entry point (used by linear, conv2d, attention fallbacks)
# --------------------------------------------------------------------------
def gemm(a, b, *, ta=False, tb=False, bias=None, residual=None, act=ACT_NONE, preact=None,
         out=None, accumulate=False, split_k=0, out_dtype=None, alpha=None, cfg=-1):
    """C = act(alpha · op(A) @ op(B) + bias) + residual  (op = transpose if flag set).

    A, B are 2-D row-major bf16.  On CPU it is the ATen reference.
    ``accumulate`` adds into ``out`` (fp32 or bf16) instead of overwriting.
    ``alpha`` is an optional 1-element fp32 DEVICE tensor (read in the epilogue,
    graph-safe).  ``cfg`` forces a tile config (-1 = auto; the list is above ``rn_gemm`` in
    csrc/kernels/gemm_bf16.hip).
    """
    if _ext.use_native(a):
        return _ext.ops().gemm(a, b, ta, tb, bias, residual, act, preact, out, accumulate, split_k,
                               out_dtype == torch.float32, alpha, cfg)
    A = a.t() if ta else a
    B = b.t() if tb else b
    h = A.float() @ B.float()
    if alpha is not None:
        h = h * alpha.float()
    if bias is not None:
        h = h + bias.float()
    if act == ACT_MUL_BWD:
        h = h * preact.float()
    elif preact is not None:
        preact.copy_(_pre_ref(h, act))
    y = _act_ref(h, act)
    if residual is not None:
        y = y + residual.float()
    dt = out_dtype or (out.dtype if out is not None else a.dtype)
    if out is not None:
        if accumulate:
            out.add_(y.to(out.dtype))
        else:
            out.copy_(y)
        return out
    return y.to(dt)


def bias_act_grad(dy2d, h2d, act, want_bias):
    """dH = dY ⊙ act'(H) and db = Σ_rows dH in one pass (fused kernel on GPU)."""
    if _ext.use_native(dy2d):
        dh, db = _ext.ops().bias_act_grad(dy2d, h2d if act != ACT_NONE else None, act, want_bias)
        return dh, (db if want_bias else None)
    dh = _act_grad_ref(dy2d, h2d, act) if act != ACT_NONE else dy2d
    db = dh.float().sum(0) if want_bias else None
    return dh, db


def _direct_grad(p):
    """The flat-buffer ``.grad`` view of parameter ``p`` if its gradient may be
    accumulated directly by a backward kernel (GEMM epilogue / reduction with
    ``accumulate``), bypassing autograd's AccumulateGrad add.  Parameters used
    once per forward qualify; a shared (tied) parameter qualifies when it
    declares how many direct contributions a backward makes (``_rn_direct_uses``,
    e.g. 2 for GPT-2's token embedding + LM head)."""
    f = getattr(p, "_rn_flat", None)
    if f is None or not f.direct or p.grad is None:
        return None
    if getattr(p, "_rn_shared", False) and getattr(p, "_rn_direct_uses", 0) < 2:
        return None
    return p.grad


def _notify(p):
    """Tell the flat buffer (and thus DDP's bucketing) that ``p``'s gradient is
    final — for a multi-use parameter, after its last contribution.  A fused-view parameter
    (nn/attention.py ``_fused_param``) stands for its members: each of them is final."""
    members = getattr(p, "_rn_members", None)
    if members is not None:
        for m in members:
            p._rn_flat.mark_ready(m)
        return
    uses = getattr(p, "_rn_direct_uses", 1)
    if uses > 1:
        left = getattr(p, "_rn_pending", uses) - 1
        p._rn_flat.contributed(p, left == 0)  # DDP reduces each contribution of a tied parameter
        if left > 0:
            p._rn_pending = left
            return
        p._rn_pending = uses
    p._rn_flat.mark_ready(p)


def _linear_grads(plan, saved, dy, x2, weight, native, need_dx, need_dw, dyq=None, wgrad_first=False):
    """(gx, gw) of y = x2·weightᵀ from ``dy``, each on the GEMM the forward's ``plan`` names (an
    :class:`~replicann_amd.ops.fp8.Fp8Plan` over the kept operands ``saved``; both None: a bf16 layer).
    dY goes to e5m2 at most once, through the state's ``gquant`` (which picks up a producer's offer) unless
    the caller made it already (``dyq``); a backward taking neither gradient in fp8 declines the offer.
    gw is None when it was accumulated straight into the flat gradient buffer."""
    use_d = saved is not None and need_dx and plan.dgrad
    use_w = saved is not None and need_dw and plan.wgrad
    if use_d or use_w:
        from .fp8 import fp8_dgrad, fp8_wgrad
        if dyq is None:
            dyq = saved.state.gquant(dy)
    elif saved is not None and dyq is None:
        saved.state.gdecline()

    def dgrad():
        if use_d:  # e5m2 dY · the forward's e4m3 weight
            return fp8_dgrad(dyq, saved.w8, saved.ws).to(x2.dtype)
        return gemm(dy, weight, out_dtype=x2.dtype) if need_dx else None

    def wgrad():
        acc = _direct_grad(weight) if native and need_dw else None
        if acc is not None:  # accumulate straight into the flat gradient buffer
            if use_w:  # e5m2 dY · the forward's e4m3 input
                fp8_wgrad(dy, saved.x8, saved.xs, saved.state, out=acc, accumulate=True, dyq=dyq)
            else:
                gemm(dy, x2, ta=True, split_k=-1, out=acc, accumulate=True)  # split-K chosen natively
            _notify(weight)
        elif use_w:
            return fp8_wgrad(dy, saved.x8, saved.xs, saved.state, dyq=dyq).to(weight.dtype)
        elif need_dw:
            return gemm(dy, x2, ta=True, split_k=-1, out_dtype=weight.dtype)

    if wgrad_first:
        gw = wgrad()
        return dgrad(), gw
    return dgrad(), wgrad()


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, residual, fp8=None):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        res2 = residual.reshape(-1, weight.shape[0]) if residual is not None else None
        native = _ext.use_native(x2)
        preact = None
        if act != ACT_NONE:
            preact = torch.empty(x2.shape[0], weight.shape[0], device=x.device, dtype=x.dtype)
        ctx.saved8 = ctx.plan = None
        if fp8 is not None:
            from .fp8 import fp8_forward
            fp8.bwd_plan = (False, False)  # re-decided by every forward (a stale plan would skip a bf16 dY)
            if res2 is not None and not res2.is_contiguous():
                res2 = res2.contiguous()
            need_dx, need_dw = ctx.needs_input_grad[:2]
            if fp8.fp8_bwd and (need_dx or need_dw):
                # keep the e4m3 operands for the fp8 weight / data gradients, and decide here which of
                # them the backward takes in fp8 (then nothing reads dY in bf16 there)
                y, ctx.saved8 = fp8_forward(x2, weight, bias, res2, act, preact, fp8, keep=True)
                ctx.plan = ctx.saved8.plan(x2.shape[0], weight.shape[0], weight.shape[1], need_dx, need_dw)
                fp8.bwd_plan = ctx.plan.published(need_dx, need_dw)
            else:
                y = fp8_forward(x2, weight, bias, res2, act, preact, fp8)
        elif native:
            y = _ext.ops().gemm(x2, weight, tb=True, bias=bias, residual=res2, act=act, preact=preact)
        else:
            y = gemm(x2, weight, tb=True, bias=bias, residual=res2, act=act, preact=preact,
                     out_dtype=x.dtype)
        ctx.save_for_backward(x2, weight, preact)
        ctx.bias_ref = bias
        ctx.act = act
        ctx.has_bias = bias is not None
        ctx.has_res = residual is not None
        ctx.shp = shp
        return y.reshape(*shp[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, weight, preact = ctx.saved_tensors
        bias = ctx.bias_ref
        gy2 = gy.reshape(-1, weight.shape[0])
        if not gy2.is_contiguous():
            gy2 = gy2.contiguous()
        native = _ext.use_native(gy2)
        gb = None
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if want_b and getattr(bias, "_rn_bias_done", False):
            # the downstream LayerNorm backward already accumulated Σ_rows gy into bias.grad
            bias._rn_bias_done = False
            want_b = False
        db_acc = _direct_grad(bias) if (native and want_b) else None
        if native:
            dh, db = _ext.ops().bias_act_grad(gy2, preact if ctx.act != ACT_NONE else None, ctx.act, want_b, db_acc)
        else:
            dh, db = bias_act_grad(gy2, preact, ctx.act, want_b)
        saved, ctx.saved8 = ctx.saved8, None
        gx, gw = _linear_grads(ctx.plan, saved, dh, x2, weight, native, *ctx.needs_input_grad[:2])
        if gx is not None:
            gx = gx.reshape(ctx.shp)
        if want_b:
            if db_acc is not None:
                _notify(bias)
            else:
                gb = db.to(weight.dtype)
        gres = gy if ctx.has_res else None
        return gx, gw, gb, None, gres, None


def linear(x, weight, bias=None, act=None, residual=None, fp8=None):
    """y = act(x @ weightᵀ + bias) [+ residual].  ``act`` ∈ {None,'relu','gelu'}.
    ``fp8``: an :class:`~replicann_amd.ops.fp8.Fp8State` → the forward GEMM runs in e4m3."""
    a = _ACTS[act] if not isinstance(act, int) else act
    if fp8 is None and not x.is_cuda and not torch.is_grad_enabled() and residual is None and a == ACT_NONE:
        return F.linear(x, weight, bias)
    if fp8 is not None:
        fp8.enter()
    return _LinearFn.apply(x, weight, bias, a, residual, fp8)


def linear_kv_append(x, weight, bias, kv, pos):
    """Decode-step QKV projection: y = x·weightᵀ + bias for one new token per batch row (x (B, 1, K)),
    and y's last 2·H·D columns (keys, values) written into the KV cache buffer ``kv`` (B, L, 2, H, D)
    at the device-side row ``pos`` (int64): 1 element = one row shared by the batch, B elements = row
    ``pos[b]`` for batch row b (a position outside [0, L) appends nothing).  Inference only.  On the
    GPU one launch: the append is part of the skinny GEMM's epilogue (``torch.ops.replicann.linear_kv``)."""
    B = x.shape[0]
    if pos.numel() not in (1, B):
        raise ValueError(f"linear_kv_append: pos must have 1 or {B} elements, got {pos.numel()}")
    if (_ext.use_native(x) and x.dim() == 3 and x.shape[1] == 1 and B <= 64 and not torch.is_grad_enabled()
            and kv.is_contiguous()):
        return _ext.ops().linear_kv(x.reshape(B, -1).contiguous(), weight, bias, kv,
                                    pos.reshape(-1).contiguous()).view(B, 1, -1)
    y = linear(x, weight, bias)
    w = kv[0, 0].numel()
    new = y[..., -w:].reshape(B, y.shape[1], *kv.shape[2:])
    if pos.numel() == 1:
        kv.index_copy_(1, pos.reshape(1), new)
        return y
    # one row per batch row: a scatter along dim 1; a row whose position is out of range keeps the
    # cache row it is pointed at instead (nothing appended, and no out-of-range index on the device)
    L = kv.shape[1]
    p = pos.reshape(B, 1, 1, 1, 1)
    idx = p.clamp(0, L - 1).expand(B, 1, *kv.shape[2:])
    kv.scatter_(1, idx, torch.where((p >= 0) & (p < L), new.to(kv.dtype), kv.gather(1, idx)))
    return y


# --------------------------------------------------------------------------
# fused two-layer MLP: y = act(x·W1ᵀ + b1)·W2ᵀ + b2 (+ residual)
# --------------------------------------------------------------------------
ACT_BWD = {ACT_RELU: 3, ACT_GELU: 4}  # GEMM epilogue codes: out = (A·B) ⊙ act'(pre)
# The MLP's GELU saves gelu'(h) (forward epilogue code 5) and its dgrad multiplies by it (code 6)
_MLP_FWD_ACT = {ACT_RELU: ACT_RELU, ACT_GELU: ACT_GELU_D}
_MLP_BWD_ACT = {ACT_RELU: 3, ACT_GELU: ACT_MUL_BWD}


def _bias_grad(g2, bias, native):
    """Σ_rows g2 into ``bias``'s gradient: (returned grad or None, done_direct)."""
    if bias is None or not bias.requires_grad:
        return None
    if getattr(bias, "_rn_bias_done", False):  # reduced by the downstream LayerNorm backward
        bias._rn_bias_done = False
        return None
    acc = _direct_grad(bias) if native else None
    if native:
        _, db = _ext.ops().bias_act_grad(g2, None, ACT_NONE, True, acc)
    else:
        db = g2.float().sum(0)
    if acc is not None:
        _notify(bias)
        return None
    return db.to(bias.dtype)


class _MLPFn(torch.autograd.Function):
    """One autograd node for the whole MLP so the activation backward runs in the
    epilogue of the second layer's dgrad GEMM:  dH = (dY·W2) ⊙ act'(pre)  — the
    separate activation-backward pass over dU (read dU + pre, write dH) is gone."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act, residual, fp8=None):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        res2 = residual.reshape(-1, w2.shape[0]).contiguous() if residual is not None else None
        ops = _ext.ops()
        nig = ctx.needs_input_grad
        # (tokens, n_out, n_in) of the two layers; layer 2's data gradient dU is always computed
        dims1, dims2 = (x2.shape[0], w1.shape[0], w1.shape[1]), (x2.shape[0], w2.shape[0], w1.shape[0])
        need1, need2 = (nig[0], nig[1]), (True, nig[3])
        pre = torch.empty(x2.shape[0], w1.shape[0], device=x.device, dtype=x.dtype)
        sv1 = sv2 = None
        if fp8 is not None:  # (state of layer 1, state of layer 2 or None): e4m3 forward GEMMs
            from .fp8 import fp8_forward
            f1, f2 = fp8
            for st in fp8:  # re-decided by every forward (a stale plan would skip a bf16 dY)
                if st is not None:
                    st.bwd_plan = (False, False)
        ctx.pre_is_h = fp8 is not None and f2 is not None and _MLPFn._fp8_keep_h(
            act, f2, f1.plan(*dims1, *need1), f2.plan(*dims2, *need2), nig, dims1[1], x2.device)
        if ctx.pre_is_h:
            # the all-fp8 MLP (both layers' fp8 gradients, fused backward): c_fc on the one-wave-per-SIMD
            # fp8 GEMM writes h = x·W1ᵀ + b1 only, ONE pass makes e4m3(gelu(h)) for the MLP c_proj
            # (ops gelu_q8, the consumer's delayed scale), and the backward re-derives gelu'(h) inside its
            # fused e5m2 pass: gelu(h) / gelu'(h) are never written in bf16
            h, sv1 = fp8_forward(x2, w1, b1, None, ACT_NONE, None, f1, keep=True)
            slot = f2.roll_slot(0)
            f2.offer(h, ops.gelu_q8(h, slot), slot)
            f2.bwd_plan = (True, True)  # the fused backward takes dY in e5m2 (a producer may offer it)
            y, sv2 = fp8_forward(h, w2, b2, res2, ACT_NONE, None, f2, keep=True)
            pre = u = h  # ("u" only lends its shape to the backward)
        elif fp8 is not None:
            # layer 2's e4m3 input comes out of layer 1's epilogue (its delayed scale permitting)
            # the e4m3 operands are kept for the fp8 weight gradients and layer 1's fp8 data gradient
            # (layer 2's data gradient carries the fused activation backward: bf16)
            if (nig[1] and f1.wgrad) or (nig[0] and f1.dgrad):
                u, sv1 = fp8_forward(x2, w1, b1, None, _MLP_FWD_ACT[act], pre, f1, out8=f2, keep=True)
            else:
                u = fp8_forward(x2, w1, b1, None, _MLP_FWD_ACT[act], pre, f1, out8=f2)
            if f2 is not None and ((nig[3] and f2.wgrad) or f2.dgrad):
                # (the e4m3 weight also for layer 2's fp8 data gradient: see _MLPFn._fp8_backward)
                y, sv2 = fp8_forward(u, w2, b2, res2, ACT_NONE, None, f2, keep=True)
            elif f2 is not None:
                y = fp8_forward(u, w2, b2, res2, ACT_NONE, None, f2)
            else:
                y = ops.gemm(u, w2, tb=True, bias=b2, residual=res2)
        else:
            u = ops.gemm(x2, w1, tb=True, bias=b1, act=_MLP_FWD_ACT[act], preact=pre)
            y = ops.gemm(u, w2, tb=True, bias=b2, residual=res2)
        # each layer's plan from what its forward kept: the backward executes them
        p1 = sv1.plan(*dims1, *need1) if sv1 is not None else None
        p2 = sv2.plan(*dims2, *need2) if sv2 is not None else None
        ctx.saved8, ctx.plans = (sv1, sv2), (p1, p2)
        ctx.fused = _MLPFn._fp8_fusable(act, p1, p2, nig, dims1[1])
        ctx.save_for_backward(x2, w1, pre, u, w2)
        ctx.b1, ctx.b2, ctx.act, ctx.shp, ctx.has_res = b1, b2, act, shp, residual is not None
        return y.reshape(*shp[:-1], w2.shape[0])

    @staticmethod
    def _fp8_fusable(act, p1, p2, nig, n_hidden):
        """:meth:`_fp8_backward` serves these plans: GELU, x and W1 need gradients, both data gradients and
        layer 1's weight gradient on the fp8 GEMMs, a hidden width its fused e5m2 pass vectorises over."""
        from .fp8 import FP8_MLP_FUSE
        return bool(FP8_MLP_FUSE and p1 is not None and p2 is not None and _MLP_FWD_ACT.get(act) == ACT_GELU_D
                    and nig[0] and nig[1] and p1.wgrad and p1.dgrad and p2.dgrad and n_hidden % 8 == 0)

    @staticmethod
    def _fp8_keep_h(act, f2, p1, p2, nig, n_hidden, device):
        """The forward may keep h instead of gelu(h) / gelu'(h) only when the backward is certain to take the
        fused fp8 path (which reads neither) with BOTH weight gradients on the fp8 GEMM too (the bf16 fallback
        would read h for gelu(h) in c_proj's and dU for dH in c_fc's: ADVICE r5, high), in training, with the
        consumer's delayed scale already seeded."""
        return (_MLPFn._fp8_fusable(act, p1, p2, nig, n_hidden) and p2.wgrad and f2.producer_ready(device)
                and not f2.inference())

    @staticmethod
    def _fp8_backward(ctx, gy, gy2, x2, w1, pre, u, w2, sv1, sv2, p1, p2):
        """Both layers' gradients in fp8 with the GELU backward fused into the e5m2 quantisation of
        dH: dY → e5m2 once (layer 2's dgrad + wgrad), dU = dY·W2 on the fp8 dgrad GEMM, then ONE pass
        dH8 = e5m2(dU ⊙ gelu'(h)) that also reduces layer 1's bias gradient (csrc/kernels/fp8.hip
        act_mul_bf8_k), and layer 1's fp8 dgrad / wgrad from dH8.  Replaces the bf16 dgrad GEMM with
        the multiply in its epilogue + the separate e5m2 pass over dH (profiles/gpt2m_fp8_r5g.txt).
        Taken when the forward found the two plans fusable (``ctx.fused``)."""
        nig = ctx.needs_input_grad
        dyq2 = sv2.state.gquant(gy2)  # one e5m2 dY for layer 2's wgrad and (after the bias reduction) dgrad
        _, gw2 = _linear_grads(p2, sv2, gy2, u, w2, True, False, nig[3], dyq=dyq2)
        gb2 = _bias_grad(gy2, ctx.b2, True) if nig[4] else None
        du, _ = _linear_grads(p2, sv2, gy2, u, w2, True, True, False, dyq=dyq2)
        b1 = ctx.b1
        b1_acc, gb1 = None, None
        if nig[2] and b1 is not None:
            if not getattr(b1, "_rn_bias_done", False):
                b1_acc = _direct_grad(b1)
            if b1_acc is None:
                gb1 = torch.zeros(b1.shape, device=b1.device, dtype=torch.bfloat16)
        dyq = sv1.state.gquant_mul(du, pre, b1_acc if b1_acc is not None else gb1, from_h=ctx.pre_is_h)
        if b1_acc is not None:
            _notify(b1)
        elif gb1 is not None:
            gb1 = gb1.to(b1.dtype)
        # (du: the dH shape; dH itself exists only in e5m2)
        gx, gw1 = _linear_grads(p1, sv1, du, x2, w1, True, True, True, dyq=dyq, wgrad_first=True)
        return gx.reshape(ctx.shp), gw1, gb1, gw2, gb2, None, gy if ctx.has_res else None, None

    @staticmethod
    def backward(ctx, gy):
        x2, w1, pre, u, w2 = ctx.saved_tensors
        ops = _ext.ops()
        gy2 = gy.reshape(-1, w2.shape[0]).contiguous()
        nig = ctx.needs_input_grad
        (sv1, sv2), (p1, p2) = ctx.saved8, ctx.plans
        ctx.saved8 = (None, None)
        if ctx.pre_is_h:  # the forward kept h: only the fused backward can take it (_fp8_keep_h) ...
            assert ctx.fused and sv1.x8 is not None and sv2.x8 is not None
            # ... and both weight gradients must run on the fp8 GEMM (the bf16 fallback would read h / dU)
            assert p1.wgrad and p2.wgrad, "keep-h MLP without fp8 weight gradients"
        if ctx.fused:
            return _MLPFn._fp8_backward(ctx, gy, gy2, x2, w1, pre, u, w2, sv1, sv2, p1, p2)
        _, gw2 = _linear_grads(p2, sv2, gy2, u, w2, True, False, nig[3])
        gb2 = _bias_grad(gy2, ctx.b2, True) if nig[4] else None
        b1 = ctx.b1
        b1_acc = None
        if nig[2] and b1 is not None and not getattr(b1, "_rn_bias_done", False):
            b1_acc = _direct_grad(b1)
        # dH = (dY·W2) ⊙ act'(pre); with a flat-buffer b1 its gradient Σ_rows dH comes from the
        # same GEMM's epilogue (per-tile column partials + one small reduction)
        dh = ops.gemm(gy2, w2, act=_MLP_BWD_ACT[ctx.act], preact=pre, bias_grad=b1_acc)
        if b1_acc is not None:
            _notify(b1)
            gb1 = None
        else:
            gb1 = _bias_grad(dh, b1, True) if nig[2] else None
        gx, gw1 = _linear_grads(p1, sv1, dh, x2, w1, True, nig[0], nig[1], wgrad_first=True)
        return (gx.reshape(ctx.shp) if nig[0] else None, gw1, gb1, gw2, gb2, None,
                gy if ctx.has_res else None, None)


def mlp(x, w1, b1, w2, b2, act="gelu", residual=None, fp8=None):
    """act(x·W1ᵀ + b1)·W2ᵀ + b2 [+ residual] — fused backward on GPU, plain linears on CPU.
    ``fp8``: (Fp8State, Fp8State) of the two layers → e4m3 forward GEMMs."""
    a = _ACTS[act] if not isinstance(act, int) else act
    if _ext.use_native(x) and a in ACT_BWD:
        if fp8 is not None:
            for st in fp8:
                if st is not None:
                    st.enter()
        return _MLPFn.apply(x, w1, b1, w2, b2, a, residual, fp8)
    f1, f2 = fp8 if fp8 is not None else (None, None)
    return linear(linear(x, w1, b1, act=a, fp8=f1), w2, b2, residual=residual, fp8=f2)
