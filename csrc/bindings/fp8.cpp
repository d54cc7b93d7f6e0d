// FP8 bindings: quantise / dequantise (e4m3 and e5m2), the fused fp8 producers and the fp8 GEMMs
// (kernels: fp8.hip and the GEMM units it dispatches to).
#include "binding_util.h"
#include "rn_api.h"

namespace {

std::tuple<Tensor, Tensor> fp8_quantize(const Tensor& x) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    Tensor q = at::empty(x.sizes(), x.options().dtype(at::kByte));
    Tensor state = at::empty({4}, x.options().dtype(at::kFloat));
    rn_fp8_quantize(x.data_ptr(), x.numel(), q.data_ptr(), state.data_ptr<float>(), cur_stream());
    return {q, state};
}
// delayed scaling: `state` (fp32 [4], persistent per tensor) carries the amax of the previous
// quantisation; one pass over x (the two-pass fp8_quantize initialises it)
Tensor fp8_quantize_delayed(const Tensor& x, const Tensor& state) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    TORCH_CHECK(state.scalar_type() == at::kFloat && state.numel() >= 4 && state.is_cuda());
    Tensor q = at::empty(x.sizes(), x.options().dtype(at::kByte));
    rn_fp8_quantize_delayed(x.data_ptr(), x.numel(), q.data_ptr(), state.data_ptr<float>(), cur_stream());
    return q;
}
// e5m2 ("bf8") quantisation of a gradient operand: delayed scaling (roll + one pass) or, for a slot
// without a scale yet, current scaling; state: [scale, amax, amax the scale came from, -]
// dH = dU ⊙ d (the MLP's GELU backward against the saved gelu'(h)) written only as e5m2 with the gradient
// slot ``state`` (delayed / current scaling as bf8_quantize); with ``bias_grad`` (bf16 [N]) Σ_rows dH is
// added into it
Tensor act_mul_bf8(const Tensor& du, const Tensor& d, const Tensor& state, bool delayed, const optional<Tensor>& bias_grad,
                   bool from_h) {
    CHECK_BF16(du); CHECK_BF16(d); CHECK_CONTIG(du); CHECK_CONTIG(d); GUARD(du);
    TORCH_CHECK(du.dim() == 2 && du.sizes() == d.sizes() && du.size(1) % 8 == 0, "act_mul_bf8: matching [M][N] inputs, N % 8");
    TORCH_CHECK(state.scalar_type() == at::kFloat && state.numel() >= 4 && state.is_cuda() && state.device() == du.device());
    const long M = du.size(0);
    const int N = (int)du.size(1);
    Tensor q = at::empty(du.sizes(), du.options().dtype(at::kByte));
    if (M == 0) return q;
    const bool bg = has(bias_grad);
    if (bg)
        TORCH_CHECK(bias_grad->scalar_type() == at::kBFloat16 && bias_grad->numel() == N && bias_grad->is_contiguous() &&
                        bias_grad->device() == du.device(),
                    "act_mul_bf8: bias_grad must be a contiguous bf16 [N] tensor on the same device");
    const int G = rn_act_mul_bf8_groups(M, N);
    Tensor part = bg ? at::empty({(int64_t)G * N}, du.options().dtype(at::kFloat)) : Tensor();
    rn_act_mul_bf8(du.data_ptr(), d.data_ptr(), M, N, q.data_ptr(), state.data_ptr<float>(), delayed ? 1 : 0,
                   bg ? part.data_ptr<float>() : nullptr, from_h ? 1 : 0, cur_stream());
    if (bg) {
        Tensor tmp = at::empty({rn_colsum_ws(N)}, du.options().dtype(at::kFloat));
        rn_colsum_f32(part.data_ptr<float>(), G, N, tmp.data_ptr<float>(), bias_grad->data_ptr(), 1, cur_stream());
    }
    return q;
}

// e4m3(gelu(h)) with the delayed-scaling slot ``state`` (rolled here, amax recorded): see rn_gelu_q8
Tensor gelu_q8(const Tensor& h, const Tensor& state) {
    CHECK_BF16(h); CHECK_CONTIG(h); GUARD(h);
    TORCH_CHECK(state.scalar_type() == at::kFloat && state.numel() >= 4 && state.is_cuda() && state.device() == h.device());
    TORCH_CHECK(h.numel() % 8 == 0, "gelu_q8: numel % 8");
    Tensor q = at::empty(h.sizes(), h.options().dtype(at::kByte));
    if (h.numel()) rn_gelu_q8(h.data_ptr(), h.numel(), q.data_ptr(), state.data_ptr<float>(), cur_stream());
    return q;
}

Tensor bf8_quantize(const Tensor& x, const Tensor& state, bool delayed) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    TORCH_CHECK(state.scalar_type() == at::kFloat && state.numel() >= 4 && state.is_cuda());
    Tensor q = at::empty(x.sizes(), x.options().dtype(at::kByte));
    rn_bf8_quantize(x.data_ptr(), x.numel(), q.data_ptr(), state.data_ptr<float>(), delayed ? 1 : 0, cur_stream());
    return q;
}
Tensor bf8_dequantize(const Tensor& q, const Tensor& state) {
    GUARD(q);
    Tensor y = at::empty(q.sizes(), q.options().dtype(at::kBFloat16));
    rn_bf8_dequantize(q.data_ptr(), q.numel(), state.data_ptr<float>(), y.data_ptr(), cur_stream());
    return y;
}
// fp8 weight gradient: out[M,N] (+)= sa·sb · a8ᵀ · b8 with a8 [K][M] (e5m2 if a_bf8, else e4m3) and
// b8 [K][N] e4m3, K = tokens (csrc/include/gemm_pk.h, fp8 MN-contiguous operands)
void gemm_fp8_wgrad(const Tensor& a8, const Tensor& b8, const Tensor& sa, const Tensor& sb, const Tensor& out,
                    bool accumulate, bool a_bf8, const optional<Tensor>& post) {
    GUARD(a8);
    TORCH_CHECK(a8.scalar_type() == at::kByte && b8.scalar_type() == at::kByte, "fp8 operands are uint8 storage");
    TORCH_CHECK(a8.dim() == 2 && b8.dim() == 2 && a8.size(0) == b8.size(0) && a8.stride(1) == 1 && b8.stride(1) == 1);
    const int K = a8.size(0), M = a8.size(1), N = b8.size(1);
    TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == N && out.stride(1) == 1);
    TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat);
    Tensor ws = at::empty({rn_gemm_fp8_wgrad_ws(M, N, K)}, a8.options().dtype(at::kFloat));
    Tensor alpha = at::empty({1}, a8.options().dtype(at::kFloat));
    int rc = rn_gemm_fp8_wgrad(a8.data_ptr(), b8.data_ptr(), out.data_ptr(), sa.data_ptr<float>(), sb.data_ptr<float>(),
                               alpha.data_ptr<float>(), ws.data_ptr<float>(), M, N, K, a8.stride(0), b8.stride(0),
                               out.stride(0), accumulate ? 1 : 0, out.scalar_type() == at::kFloat ? 1 : 0, a_bf8 ? 1 : 0,
                               cur_stream(), post ? post->data_ptr<float>() : nullptr);
    TORCH_CHECK(rc == 0, "gemm_fp8_wgrad: M, N and row strides must be multiples of 16 and K of 128, got M=", M,
                " N=", N, " K=", K);
}
// fp8 data gradient: dY8 [M][K] (e5m2 if a_bf8) · W8 [K][N] (the e4m3 weight as stored) -> bf16 [M][N]
Tensor gemm_fp8_dgrad(const Tensor& a8, const Tensor& b8, const Tensor& sa, const Tensor& sb, bool a_bf8,
                      const optional<Tensor>& post) {
    GUARD(a8);
    TORCH_CHECK(a8.scalar_type() == at::kByte && b8.scalar_type() == at::kByte, "fp8 operands are uint8 storage");
    TORCH_CHECK(a8.dim() == 2 && b8.dim() == 2 && a8.size(1) == b8.size(0) && a8.stride(1) == 1 && b8.stride(1) == 1);
    const int M = a8.size(0), K = a8.size(1), N = b8.size(1);
    Tensor c = at::empty({M, N}, a8.options().dtype(at::kBFloat16));
    Tensor alpha = at::empty({1}, a8.options().dtype(at::kFloat));
    if (M == 0) return c;
    int rc = rn_gemm_fp8_dgrad(a8.data_ptr(), b8.data_ptr(), c.data_ptr(), sa.data_ptr<float>(), sb.data_ptr<float>(),
                               alpha.data_ptr<float>(), M, N, K, a8.stride(0), b8.stride(0), c.stride(0), a_bf8 ? 1 : 0,
                               cur_stream(), post ? post->data_ptr<float>() : nullptr);
    TORCH_CHECK(rc == 0, "gemm_fp8_dgrad: K, N and row strides must be multiples of 16, got K=", K, " N=", N);
    return c;
}
Tensor fp8_dequantize(const Tensor& q, const Tensor& state) {
    GUARD(q);
    Tensor y = at::empty(q.sizes(), q.options().dtype(at::kBFloat16));
    rn_fp8_dequantize(q.data_ptr(), q.numel(), state.data_ptr<float>(), y.data_ptr(), cur_stream());
    return y;
}
Tensor gemm_fp8(const Tensor& a8, const Tensor& b8, const Tensor& sa, const Tensor& sb, const optional<Tensor>& bias,
                const optional<Tensor>& residual, int64_t act, const optional<Tensor>& preact) {
    GUARD(a8);
    TORCH_CHECK(a8.scalar_type() == at::kByte && b8.scalar_type() == at::kByte, "fp8 operands are uint8 storage");
    TORCH_CHECK(a8.dim() == 2 && b8.dim() == 2 && a8.size(1) == b8.size(1) && a8.is_contiguous() && b8.is_contiguous());
    const int M = a8.size(0), N = b8.size(0), K = a8.size(1);
    Tensor c = at::empty({M, N}, a8.options().dtype(at::kBFloat16));
    Tensor alpha = at::empty({1}, a8.options().dtype(at::kFloat));
    if (has(residual)) { CHECK_BF16(*residual); TORCH_CHECK(residual->is_contiguous()); }
    int rc = rn_gemm_fp8(a8.data_ptr(), b8.data_ptr(), c.data_ptr(), optr(bias), optr(residual),
                         has(preact) ? preact->data_ptr() : nullptr, sa.data_ptr<float>(),
                         sb.data_ptr<float>(), alpha.data_ptr<float>(), M, N, K, a8.stride(0), b8.stride(0), c.stride(0),
                         (int)act, cur_stream(), nullptr, nullptr);
    TORCH_CHECK(rc == 0, "gemm_fp8: K and row strides must be multiples of 16, got K=", K);
    return c;
}
// gemm_fp8 whose activation output also comes out in e4m3 for the next fp8 GEMM (`q8_state`: that
// GEMM's activation Fp8State slot; delayed scaling, rolled here, amax recorded by the epilogue)
std::tuple<Tensor, Tensor> gemm_fp8_q8(const Tensor& a8, const Tensor& b8, const Tensor& sa, const Tensor& sb,
                                       const optional<Tensor>& bias, int64_t act, const Tensor& preact,
                                       const Tensor& q8_state) {
    GUARD(a8);
    TORCH_CHECK(a8.scalar_type() == at::kByte && b8.scalar_type() == at::kByte, "fp8 operands are uint8 storage");
    TORCH_CHECK(a8.dim() == 2 && b8.dim() == 2 && a8.size(1) == b8.size(1) && a8.is_contiguous() && b8.is_contiguous());
    TORCH_CHECK(q8_state.scalar_type() == at::kFloat && q8_state.numel() >= 4 && q8_state.is_cuda());
    const int M = a8.size(0), N = b8.size(0), K = a8.size(1);
    TORCH_CHECK(preact.size(0) == M && preact.size(1) == N && preact.is_contiguous());
    Tensor c = at::empty({M, N}, a8.options().dtype(at::kBFloat16));
    Tensor q = at::empty({M, N}, a8.options().dtype(at::kByte));
    Tensor alpha = at::empty({1}, a8.options().dtype(at::kFloat));
    int rc = rn_gemm_fp8(a8.data_ptr(), b8.data_ptr(), c.data_ptr(), optr(bias), nullptr, preact.data_ptr(),
                         sa.data_ptr<float>(), sb.data_ptr<float>(), alpha.data_ptr<float>(), M, N, K, a8.stride(0),
                         b8.stride(0), c.stride(0), (int)act, cur_stream(), q.data_ptr(), q8_state.data_ptr<float>());
    TORCH_CHECK(rc == 0, "gemm_fp8_q8: unsupported shape / activation (rc ", rc, ")");
    return {c, q};
}

// e4m3 copies of many weights of one flat bf16 parameter buffer, two launches (see fp8.hip)
void fp8_quant_many(const Tensor& flat, const Tensor& segs, int64_t max_n, const Tensor& qbuf, bool roll) {
    CHECK_BF16(flat); GUARD(flat);
    TORCH_CHECK(segs.scalar_type() == at::kLong && segs.is_cuda() && segs.dim() == 2 && segs.size(1) == 4 &&
                segs.is_contiguous());
    TORCH_CHECK(qbuf.scalar_type() == at::kByte && qbuf.is_cuda());
    rn_fp8_quant_many(flat.data_ptr(), segs.data_ptr<int64_t>(), (int)segs.size(0), (long)max_n, qbuf.data_ptr(),
                      roll ? 1 : 0, cur_stream());
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(replicann, m) {
    m.def("fp8_quantize(Tensor x) -> (Tensor, Tensor)");
    m.def("fp8_dequantize(Tensor q, Tensor state) -> Tensor");
    m.def("fp8_quantize_delayed(Tensor x, Tensor state) -> Tensor");
    m.def("bf8_quantize(Tensor x, Tensor(a!) state, bool delayed) -> Tensor");
    m.def("act_mul_bf8(Tensor du, Tensor d, Tensor(a!) state, bool delayed, Tensor(b!)? bias_grad=None, bool from_h=False) -> Tensor");
    m.def("gelu_q8(Tensor h, Tensor(a!) state) -> Tensor");
    m.def("bf8_dequantize(Tensor q, Tensor state) -> Tensor");
    m.def("gemm_fp8_wgrad(Tensor a8, Tensor b8, Tensor sa, Tensor sb, Tensor(a!) out, bool accumulate, bool a_bf8, "
          "Tensor? post=None) -> ()");
    m.def("gemm_fp8_dgrad(Tensor a8, Tensor b8, Tensor sa, Tensor sb, bool a_bf8, Tensor? post=None) -> Tensor");
    m.def("gemm_fp8(Tensor a8, Tensor b8, Tensor sa, Tensor sb, Tensor? bias, Tensor? residual, int act, Tensor? preact) -> Tensor");
    m.def("gemm_fp8_q8(Tensor a8, Tensor b8, Tensor sa, Tensor sb, Tensor? bias, int act, Tensor(a!) preact, Tensor(b!) q8_state) -> (Tensor, Tensor)");
    m.def("fp8_quant_many(Tensor flat, Tensor segs, int max_n, Tensor(a!) qbuf, bool roll=True) -> ()");
}

TORCH_LIBRARY_IMPL(replicann, CUDA, m) {
    m.impl("fp8_quantize", &fp8_quantize);
    m.impl("fp8_dequantize", &fp8_dequantize);
    m.impl("fp8_quantize_delayed", &fp8_quantize_delayed);
    m.impl("bf8_quantize", &bf8_quantize);
    m.impl("act_mul_bf8", &act_mul_bf8);
    m.impl("gelu_q8", &gelu_q8);
    m.impl("bf8_dequantize", &bf8_dequantize);
    m.impl("gemm_fp8_wgrad", &gemm_fp8_wgrad);
    m.impl("gemm_fp8_dgrad", &gemm_fp8_dgrad);
    m.impl("gemm_fp8", &gemm_fp8);
    m.impl("gemm_fp8_q8", &gemm_fp8_q8);
    m.impl("fp8_quant_many", &fp8_quant_many);
}
