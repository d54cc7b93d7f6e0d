// Elementwise, softmax, cross-entropy and LayerNorm bindings: activations, dropout and its device seed
// stream, add + relu, row softmax, the loss, LayerNorm (kernels: elementwise.hip, softmax_xent.hip,
// layernorm.hip).  One unit for these small families: each binding unit costs a torch-header parse.
#include "binding_util.h"
#include "rn_api.h"

namespace {

// ------------------------------------------------------------------ elementwise
Tensor act_fwd(const Tensor& x, int64_t kind) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    Tensor y = at::empty_like(x);
    rn_act_fwd(x.data_ptr(), y.data_ptr(), x.numel(), (int)kind, cur_stream());
    return y;
}
Tensor act_bwd(const Tensor& dy, const Tensor& x, int64_t kind) {
    CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_CONTIG(x); GUARD(dy);
    Tensor dx = at::empty_like(dy);
    rn_act_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), dy.numel(), (int)kind, cur_stream());
    return dx;
}
Tensor dropout_fwd(const Tensor& x, double p, int64_t seed, const optional<Tensor>& seed_buf) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    Tensor y = at::empty_like(x);
    rn_dropout(x.data_ptr(), y.data_ptr(), x.numel(), (float)p, (uint64_t)seed, seed_ptr(seed_buf), cur_stream());
    return y;
}
void rng_next(const Tensor& state, const Tensor& out) {
    TORCH_CHECK(state.scalar_type() == at::kLong && out.scalar_type() == at::kLong && state.is_cuda() && out.is_cuda());
    GUARD(state);
    rn_rng_next(state.data_ptr(), out.data_ptr(), cur_stream());
}
Tensor add_act(const Tensor& a, const Tensor& b, bool relu) {
    CHECK_BF16(a); CHECK_CONTIG(a); CHECK_CONTIG(b); GUARD(a);
    TORCH_CHECK(a.sizes() == b.sizes());
    Tensor y = at::empty_like(a);
    rn_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), relu, cur_stream());
    return y;
}

// ------------------------------------------------------------------ softmax / xent
Tensor softmax_fwd(const Tensor& x, double scale) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    Tensor y = at::empty_like(x);
    if (x.numel()) rn_softmax_fwd(x.data_ptr(), y.data_ptr(), x.size(0), x.size(1), (float)scale, cur_stream());
    return y;
}
Tensor softmax_bwd(const Tensor& dy, const Tensor& y, double scale) {
    CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_CONTIG(y); GUARD(dy);
    Tensor dx = at::empty_like(dy);
    if (dy.numel()) rn_softmax_bwd(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), y.size(0), y.size(1), (float)scale, cur_stream());
    return dx;
}
std::tuple<Tensor, Tensor> xent_fwd(const Tensor& logits, const Tensor& target, int64_t nvalid, int64_t ignore,
                                    bool write_grad) {
    CHECK_BF16(logits); CHECK_CONTIG(logits); GUARD(logits);
    TORCH_CHECK(target.scalar_type() == at::kLong && target.is_contiguous());
    const int M = logits.size(0), V = logits.size(1);
    Tensor loss = at::empty({M}, logits.options().dtype(at::kFloat));
    Tensor lse = at::empty({M}, logits.options().dtype(at::kFloat));
    if (M) rn_xent_fwd(logits.data_ptr(), target.data_ptr<int64_t>(), loss.data_ptr<float>(), lse.data_ptr<float>(), M, V,
                       (int)nvalid, (long)ignore, write_grad, cur_stream());
    return {loss, lse};
}
// the fp8 LM head's loss: as xent_fwd(write_grad) but the gradient goes to q8 (uint8 [M][V]) as e5m2 of
// (softmax - onehot) · 2^15; the logits are left unchanged
std::tuple<Tensor, Tensor> xent_fwd_q8(const Tensor& logits, const Tensor& target, int64_t nvalid, int64_t ignore,
                                       const Tensor& q8) {
    CHECK_BF16(logits); CHECK_CONTIG(logits); GUARD(logits);
    TORCH_CHECK(target.scalar_type() == at::kLong && target.is_contiguous());
    TORCH_CHECK(q8.scalar_type() == at::kByte && q8.is_contiguous() && q8.sizes() == logits.sizes());
    const int M = logits.size(0), V = logits.size(1);
    Tensor loss = at::empty({M}, logits.options().dtype(at::kFloat));
    Tensor lse = at::empty({M}, logits.options().dtype(at::kFloat));
    if (M) {
        int rc = rn_xent_fwd_q8(logits.data_ptr(), target.data_ptr<int64_t>(), loss.data_ptr<float>(),
                                lse.data_ptr<float>(), M, V, (int)nvalid, (long)ignore, q8.data_ptr(), cur_stream());
        TORCH_CHECK(rc == 0, "xent_fwd_q8: V must be a multiple of 8 and <= 65536, got ", V);
    }
    return {loss, lse};
}
void xent_bwd(const Tensor& logits, const Tensor& target, const Tensor& lse, const Tensor& gscale, const Tensor& grad,
              int64_t nvalid, int64_t ignore) {
    CHECK_BF16(logits); GUARD(logits);
    TORCH_CHECK(gscale.scalar_type() == at::kFloat && gscale.is_cuda());
    const int M = logits.size(0), V = logits.size(1);
    if (M) rn_xent_bwd(logits.data_ptr(), target.data_ptr<int64_t>(), lse.data_ptr<float>(), gscale.data_ptr<float>(),
                       grad.data_ptr(), M, V, (int)nvalid, (long)ignore, cur_stream());
}

// ------------------------------------------------------------------ layernorm
std::tuple<Tensor, Tensor, Tensor, Tensor> layernorm_fwd(const Tensor& x, const optional<Tensor>& r, const Tensor& w,
                                                         const optional<Tensor>& b, double eps) {
    CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(w); GUARD(x);
    const int M = x.size(0), E = x.size(1);
    Tensor y = at::empty_like(x);
    Tensor h = has(r) ? at::empty_like(x) : x;
    Tensor mean = at::empty({M}, x.options().dtype(at::kFloat));
    Tensor rstd = at::empty({M}, x.options().dtype(at::kFloat));
    if (M) {
        int rc = rn_ln_fwd(x.data_ptr(), optr(r), w.data_ptr(), optr(b), y.data_ptr(), h.data_ptr(), mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), M, E, (float)eps, cur_stream(), nullptr, nullptr);
        TORCH_CHECK(rc == 0, "layernorm: E must be a multiple of 8 and <= 8192, got ", E);
    }
    return {y, h, mean, rstd};
}
// LayerNorm whose output also comes out as e4m3 for the consumer's fp8 GEMM: `state` is that
// GEMM's activation Fp8State slot (delayed scaling: rolled here, amax recorded by the kernel)
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> layernorm_fwd_q8(const Tensor& x, const optional<Tensor>& r,
                                                                    const Tensor& w, const optional<Tensor>& b,
                                                                    double eps, const Tensor& state) {
    CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(w); GUARD(x);
    TORCH_CHECK(state.scalar_type() == at::kFloat && state.numel() >= 4 && state.is_cuda() && state.is_contiguous());
    const int M = x.size(0), E = x.size(1);
    Tensor y = at::empty_like(x);
    Tensor h = has(r) ? at::empty_like(x) : x;
    Tensor mean = at::empty({M}, x.options().dtype(at::kFloat));
    Tensor rstd = at::empty({M}, x.options().dtype(at::kFloat));
    Tensor q = at::empty(x.sizes(), x.options().dtype(at::kByte));
    rn_fp8_roll(state.data_ptr<float>(), cur_stream());
    if (M) {
        int rc = rn_ln_fwd(x.data_ptr(), optr(r), w.data_ptr(), optr(b), y.data_ptr(), h.data_ptr(), mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), M, E, (float)eps, cur_stream(), q.data_ptr(), state.data_ptr<float>());
        TORCH_CHECK(rc == 0, "layernorm: E must be a multiple of 8 and <= 8192, got ", E);
    }
    return {y, h, mean, rstd, q};
}
std::tuple<Tensor, Tensor, Tensor> layernorm_bwd(const Tensor& dy, const optional<Tensor>& gh, const Tensor& h,
                                                 const Tensor& w, const Tensor& mean, const Tensor& rstd,
                                                 const optional<Tensor>& dw_accum, const optional<Tensor>& db_accum,
                                                 const optional<Tensor>& dxs_accum, const optional<Tensor>& q8,
                                                 const optional<Tensor>& q8_state) {
    CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_CONTIG(h); GUARD(dy);
    if (has(dxs_accum)) {
        CHECK_BF16(*dxs_accum);
        TORCH_CHECK(dxs_accum->numel() == dy.size(1) && dxs_accum->is_contiguous());
    }
    const int M = dy.size(0), E = dy.size(1);
    Tensor dx = at::empty_like(dy);
    const bool accum = has(dw_accum) && has(db_accum);
    Tensor dw = accum ? *dw_accum : at::empty({E}, w.options());  // parameter dtype (bf16)
    Tensor db = accum ? *db_accum : at::empty({E}, w.options());
    Tensor part = at::empty({rn_ln_bwd_ws(M, E)}, dy.options().dtype(at::kFloat));
    // q8 + q8_state: dx also in e5m2 for the fp8 linear that produced the LayerNorm input (its gradient slot)
    void* q8_ptr = nullptr;
    float* q8_st = nullptr;
    if (has(q8)) {
        TORCH_CHECK(q8->scalar_type() == at::kByte && q8->is_contiguous() && q8->numel() == dy.numel() &&
                    q8->device() == dy.device(), "layernorm_bwd: q8 must be a contiguous uint8 twin of dy");
        TORCH_CHECK(has(q8_state) && q8_state->scalar_type() == at::kFloat && q8_state->numel() >= 4 &&
                    q8_state->device() == dy.device(), "layernorm_bwd: q8 needs a 4-float fp32 scale slot");
        q8_ptr = q8->data_ptr();
        q8_st = q8_state->data_ptr<float>();
    }
    if (M) {
        int rc = rn_ln_bwd(dy.data_ptr(), optr(gh), h.data_ptr(), w.data_ptr(), mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), dx.data_ptr(), nullptr, nullptr, dw.data_ptr(), db.data_ptr(),
                           has(dxs_accum) ? dxs_accum->data_ptr() : nullptr,
                           part.data_ptr<float>(), M, E, accum, cur_stream(), q8_ptr, q8_st);
        TORCH_CHECK(rc == 0, "layernorm_bwd: unsupported E=", E);
    } else if (!accum) { dw.zero_(); db.zero_(); }
    return {dx, dw, db};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(replicann, m) {
    m.def("act_fwd(Tensor x, int kind) -> Tensor");
    m.def("act_bwd(Tensor dy, Tensor x, int kind) -> Tensor");
    m.def("dropout_fwd(Tensor x, float p, int seed, Tensor? seed_buf=None) -> Tensor");
    m.def("rng_next(Tensor(a!) state, Tensor(b!) out) -> ()");
    m.def("add_act(Tensor a, Tensor b, bool relu) -> Tensor");
    m.def("softmax_fwd(Tensor x, float scale) -> Tensor");
    m.def("softmax_bwd(Tensor dy, Tensor y, float scale) -> Tensor");
    m.def("xent_fwd(Tensor(a!) logits, Tensor target, int nvalid, int ignore, bool write_grad=False) -> (Tensor, Tensor)");
    m.def("xent_fwd_q8(Tensor logits, Tensor target, int nvalid, int ignore, Tensor(a!) q8) -> (Tensor, Tensor)");
    m.def("xent_bwd(Tensor logits, Tensor target, Tensor lse, Tensor gscale, Tensor(a!) grad, int nvalid, int ignore) -> ()");
    m.def("layernorm_fwd(Tensor x, Tensor? r, Tensor w, Tensor? b, float eps) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("layernorm_fwd_q8(Tensor x, Tensor? r, Tensor w, Tensor? b, float eps, Tensor(a!) state) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("layernorm_bwd(Tensor dy, Tensor? gh, Tensor h, Tensor w, Tensor mean, Tensor rstd, "
          "Tensor(a!)? dw_accum=None, Tensor(b!)? db_accum=None, Tensor(c!)? dxs_accum=None, Tensor(d!)? q8=None, "
          "Tensor(e!)? q8_state=None) -> (Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(replicann, CUDA, m) {
    m.impl("act_fwd", &act_fwd);
    m.impl("act_bwd", &act_bwd);
    m.impl("dropout_fwd", &dropout_fwd);
    m.impl("rng_next", &rng_next);
    m.impl("add_act", &add_act);
    m.impl("softmax_fwd", &softmax_fwd);
    m.impl("softmax_bwd", &softmax_bwd);
    m.impl("xent_fwd", &xent_fwd);
    m.impl("xent_fwd_q8", &xent_fwd_q8);
    m.impl("xent_bwd", &xent_bwd);
    m.impl("layernorm_fwd", &layernorm_fwd);
    m.impl("layernorm_fwd_q8", &layernorm_fwd_q8);
    m.impl("layernorm_bwd", &layernorm_bwd);
}
