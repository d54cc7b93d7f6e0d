// Convolution-network bindings: implicit-GEMM conv, im2col / col2im, pooling, BatchNorm
// (kernels: gemm_conv.hip, conv3x3.hip, conv.hip).
#include <cstdlib>

#include "binding_util.h"
#include "rn_api.h"

namespace {

// ------------------------------------------------------------------ implicit-GEMM conv
// x / dy NHWC bf16 contiguous, w (OC, KH, KW, C) contiguous; the gathered tensor's channel count
// must be a multiple of 64 (callers check conv_implicit_ok first).
// stats: also return [ceil(M/256)][2·OC] fp32 per-256-row Σ | Σ² of y (the following BatchNorm's batch
// statistics, reduced in batchnorm_fwd instead of re-reading y)
static std::tuple<Tensor, Tensor> conv_fwd_implicit_impl(const Tensor& x, const Tensor& w,
                                                         const optional<Tensor>& bias, int64_t S, int64_t P,
                                                         bool stats) {
    CHECK_BF16(x); CHECK_CONTIG(x); CHECK_BF16(w); CHECK_CONTIG(w); GUARD(x);
    const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    const int OC = w.size(0), KH = w.size(1), KW = w.size(2);
    TORCH_CHECK(w.size(3) == C, "conv: channel mismatch");
    const int OH = (H + 2 * P - KH) / S + 1, OW = (W + 2 * P - KW) / S + 1;
    Tensor y = at::empty({N, OH, OW, OC}, x.options());
    const int M = N * OH * OW, K = KH * KW * C;
    // 3×3 / stride 1 / pad 1, 64 → 64 channels (ResNet layer 1): the halo-tile kernel (conv3x3.hip); its
    // statistics partials are per tile of whole image rows instead of per 256 pixels
    const bool has_bias = has(bias);
    if (KH == 3 && KW == 3 && S == 1 && P == 1 && C == 64 && OC == 64 && !has_bias && M > 0) {
        const int tiles = rn_conv3x3_tiles(N, H, W);
        if (tiles > 0) {
            Tensor part3 = stats ? at::empty({tiles, 2L * OC}, x.options().dtype(at::kFloat))
                                 : at::empty({0}, x.options().dtype(at::kFloat));
            if (rn_conv3x3(x.data_ptr(), w.data_ptr(), y.data_ptr(), stats ? part3.data_ptr<float>() : nullptr, N, H,
                           W, 0, 0, cur_stream()) == 0)
                return {y, part3};
        }
    }
    Tensor part = stats ? at::empty({(M + 255) / 256, 2L * OC}, x.options().dtype(at::kFloat))
                        : at::empty({0}, x.options().dtype(at::kFloat));
    if (M == 0) return {y, part};
    float* cp = stats ? part.data_ptr<float>() : nullptr;
    if (has(bias)) { CHECK_BF16(*bias); TORCH_CHECK(bias->numel() == OC); }
    const int rc = rn_conv_gemm(1, x.data_ptr(), w.data_ptr(), y.data_ptr(), optr(bias), nullptr, M, OC, K, 0, K, OC, H,
                                W, C, OH, OW, KH, KW, (int)S, (int)P, C, 0, 0, 1, 0, 0, cp, cur_stream());
    TORCH_CHECK(rc == 0, "implicit conv fwd: unsupported geometry");
    return {y, part};
}
Tensor conv_fwd_implicit(const Tensor& x, const Tensor& w, const optional<Tensor>& bias, int64_t S, int64_t P) {
    return std::get<0>(conv_fwd_implicit_impl(x, w, bias, S, P, false));
}
std::tuple<Tensor, Tensor> conv_fwd_implicit_stats(const Tensor& x, const Tensor& w, const optional<Tensor>& bias,
                                                   int64_t S, int64_t P) {
    return conv_fwd_implicit_impl(x, w, bias, S, P, true);
}
// out + accumulate: dx is added into `out` in the GEMM epilogue (a second gradient of the same input)
static Tensor grad_out(const optional<Tensor>& out, bool accumulate, at::IntArrayRef shape, const Tensor& like,
                       const char* what) {
    if (has(out)) {
        CHECK_BF16(*out); CHECK_CONTIG(*out);
        TORCH_CHECK(out->sizes() == shape && out->device() == like.device(), what, ": out shape");
        return *out;
    }
    TORCH_CHECK(!accumulate, what, ": accumulate needs out");
    return at::empty(shape, like.options());
}
Tensor conv_dgrad_implicit(const Tensor& dy, const Tensor& w, int64_t H, int64_t W, int64_t P, const optional<Tensor>& out,
                           bool accumulate) {  // stride 1
    CHECK_BF16(dy); CHECK_CONTIG(dy); CHECK_BF16(w); CHECK_CONTIG(w); GUARD(dy);
    const int N = dy.size(0), OH = dy.size(1), OW = dy.size(2), OC = dy.size(3);
    const int KH = w.size(1), KW = w.size(2), C = w.size(3);
    TORCH_CHECK(w.size(0) == OC && OH == H + 2 * P - KH + 1 && OW == W + 2 * P - KW + 1, "conv dgrad geometry");
    Tensor dx = grad_out(out, accumulate, {N, H, W, C}, dy, "conv dgrad");
    const int M = N * (int)H * (int)W, K = KH * KW * OC;
    if (M == 0) return dx;
    if (KH == 3 && KW == 3 && P == 1 && C == 64 && OC == 64 &&
        rn_conv3x3(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), nullptr, N, (int)H, (int)W, 1, accumulate ? 1 : 0,
                   cur_stream()) == 0)
        return dx;  // the halo-tile kernel (conv3x3.hip), flipped / transposed weights
    const int rc = rn_conv_gemm(2, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), nullptr, nullptr, M, C, K, 0, 0, C, OH,
                                OW, OC, (int)H, (int)W, KH, KW, 1, (int)P, OC, C, (long)KH * KW * C, 1, 0,
                                accumulate ? 1 : 0, nullptr, cur_stream());
    TORCH_CHECK(rc == 0, "implicit conv dgrad: unsupported geometry");
    return dx;
}
Tensor conv_wgrad_implicit(const Tensor& dy2, const Tensor& x, int64_t KH, int64_t KW, int64_t S, int64_t P,
                           const optional<Tensor>& out, bool accumulate) {
    CHECK_BF16(dy2); CHECK_CONTIG(dy2); CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    const int OH = (H + 2 * P - KH) / S + 1, OW = (W + 2 * P - KW) / S + 1;
    const int OC = dy2.size(1), PIX = N * OH * OW, K = KH * KW * C;
    TORCH_CHECK(dy2.size(0) == PIX, "conv wgrad: dy rows != output pixels");
    Tensor dw;
    if (has(out)) {  // e.g. the flat gradient view of the weight (accumulate: direct grad)
        CHECK_BF16(*out); CHECK_CONTIG(*out);
        TORCH_CHECK(out->numel() == (long)OC * K && out->device() == x.device(), "conv wgrad: out shape");
        dw = *out;
    } else {
        TORCH_CHECK(!accumulate, "conv wgrad: accumulate needs out");
        dw = at::empty({OC, K}, x.options());
    }
    // split-K over the pixels so the (OC/128)×(K/128) tile grid fills the chip
    int bm, bn;
    rn_conv_wgrad_tile(OC, K, &bm, &bn);
    const long tiles = (long)((OC + bm - 1) / bm) * ((K + bn - 1) / bn);
    int split = 1;
    static const long target = [] {  // workgroups to aim for (REPLICANN_CONVW_TARGET: A/B only)
        const char* e = getenv("REPLICANN_CONVW_TARGET");
        return e ? atol(e) : 512L;
    }();
    while (tiles * split < target && PIX / (split * 2) >= 1024) split *= 2;
    Tensor ws = split > 1 ? at::empty({(long)split * OC * K}, x.options().dtype(at::kFloat)) : Tensor();
    const int rc = rn_conv_gemm(3, dy2.data_ptr(), x.data_ptr(), dw.data_ptr(), nullptr,
                                ws.defined() ? ws.data_ptr<float>() : nullptr, OC, K, PIX, OC, 0, K, H, W, C, OH, OW,
                                (int)KH, (int)KW, (int)S, (int)P, C, 0, 0, split, 0, accumulate ? 1 : 0,
                                nullptr, cur_stream());
    TORCH_CHECK(rc == 0, "implicit conv wgrad: unsupported geometry");
    return dw;
}

// ------------------------------------------------------------------ conv / pool / bn
Tensor im2col(const Tensor& x, int64_t KH, int64_t KW, int64_t S, int64_t P, int64_t Kp) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    const int OH = (H + 2 * P - KH) / S + 1, OW = (W + 2 * P - KW) / S + 1;
    Tensor cols = at::empty({(int64_t)N * OH * OW, Kp}, x.options());
    rn_im2col(x.data_ptr(), cols.data_ptr(), N, H, W, C, KH, KW, S, P, OH, OW, Kp, cur_stream());
    return cols;
}
Tensor col2im(const Tensor& dcols, int64_t N, int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW, int64_t S,
              int64_t P, int64_t Kp, const optional<Tensor>& out, bool accumulate) {
    CHECK_BF16(dcols); CHECK_CONTIG(dcols); GUARD(dcols);
    const int OH = (H + 2 * P - KH) / S + 1, OW = (W + 2 * P - KW) / S + 1;
    Tensor dx = grad_out(out, accumulate, {N, H, W, C}, dcols, "col2im");
    rn_col2im(dcols.data_ptr(), dx.data_ptr(), N, H, W, C, KH, KW, S, P, OH, OW, Kp, accumulate ? 1 : 0, cur_stream());
    return dx;
}
std::tuple<Tensor, Tensor> maxpool_fwd(const Tensor& x, int64_t K, int64_t S, int64_t P) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    TORCH_CHECK(K * K <= 256, "maxpool: window too large for byte indices");
    const int N = x.size(0), H = x.size(1), W = x.size(2), C = x.size(3);
    const int OH = (H + 2 * P - K) / S + 1, OW = (W + 2 * P - K) / S + 1;
    Tensor y = at::empty({N, OH, OW, C}, x.options());
    Tensor idx = at::empty({N, OH, OW, C}, x.options().dtype(at::kByte));
    rn_maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C, K, S, P, OH, OW, cur_stream());
    return {y, idx};
}
// gy (N, OH, OW, C) + the forward's window indices → dx (N, H, W, C)
Tensor maxpool_bwd(const Tensor& gy, const Tensor& idx, int64_t H, int64_t W, int64_t K, int64_t S, int64_t P) {
    CHECK_BF16(gy); CHECK_CONTIG(gy); GUARD(gy);
    TORCH_CHECK(idx.scalar_type() == at::kByte && idx.sizes() == gy.sizes() && idx.is_contiguous());
    const int N = gy.size(0), OH = gy.size(1), OW = gy.size(2), C = gy.size(3);
    Tensor dx = at::empty({N, H, W, C}, gy.options());
    rn_maxpool_bwd(gy.data_ptr(), idx.data_ptr(), dx.data_ptr(), N, (int)H, (int)W, C, K, S, P, OH, OW, cur_stream());
    return dx;
}
Tensor avgpool_fwd(const Tensor& x) {
    CHECK_BF16(x); CHECK_CONTIG(x); GUARD(x);
    const int N = x.size(0), HW = x.size(1) * x.size(2), C = x.size(3);
    Tensor y = at::empty({N, C}, x.options());
    rn_avgpool_fwd(x.data_ptr(), y.data_ptr(), N, HW, C, cur_stream());
    return y;
}
Tensor avgpool_bwd(const Tensor& gy, int64_t H, int64_t W) {
    CHECK_BF16(gy); GUARD(gy);
    const int N = gy.size(0), C = gy.size(1);
    Tensor dx = at::empty({N, H, W, C}, gy.options());
    rn_avgpool_bwd(gy.contiguous().data_ptr(), dx.data_ptr(), N, H * W, C, cur_stream());
    return dx;
}
// NHWC BatchNorm over [M][C] rows (C % 8 == 0, C <= 2048); res (optional, same shape): y = relu(BN(x) + res)
static void check_bn(const Tensor& x, const optional<Tensor>& res) {
    CHECK_BF16(x); CHECK_CONTIG(x);
    TORCH_CHECK(rn_bn_supported((int)x.size(1)), "batchnorm: channels must be a multiple of 8 and <= 2048");
    if (has(res)) {
        CHECK_BF16(*res); CHECK_CONTIG(*res);
        TORCH_CHECK(res->sizes() == x.sizes(), "batchnorm residual shape");
    }
}
// returns (y, mean, rstd, mask): mask = relu'(y) bits, [M·C/8] bytes (empty without relu)
std::tuple<Tensor, Tensor, Tensor, Tensor> batchnorm_fwd(const Tensor& x, const Tensor& w, const Tensor& b,
                                                 const Tensor& rmean, const Tensor& rvar, double mom, double eps,
                                                 bool relu, const optional<Tensor>& res,
                                                 const optional<Tensor>& partials) {
    check_bn(x, res); GUARD(x);
    TORCH_CHECK(rmean.scalar_type() == at::kFloat && rvar.scalar_type() == at::kFloat, "BN running stats must be fp32");
    const int M = x.size(0), C = x.size(1);
    // partials: [R][2C] fp32 Σ | Σ² row-block partials of x from its producer (conv_fwd_implicit_stats)
    const bool hp = has(partials);
    if (hp)
        TORCH_CHECK(partials->scalar_type() == at::kFloat && partials->dim() == 2 && partials->size(1) == 2L * C &&
                        partials->is_contiguous() && partials->device() == x.device(),
                    "batchnorm_fwd: partials must be fp32 [R][2C]");
    Tensor y = at::empty_like(x);
    Tensor mean = at::empty({C}, x.options().dtype(at::kFloat));
    Tensor rstd = at::empty({C}, x.options().dtype(at::kFloat));
    Tensor ws = at::empty({rn_bn_ws_floats(M, C)}, x.options().dtype(at::kFloat));
    Tensor mask = at::empty({relu ? (int64_t)M * C / 8 : 0}, x.options().dtype(at::kByte));
    rn_bn_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), rmean.data_ptr<float>(), rvar.data_ptr<float>(), y.data_ptr(),
              mean.data_ptr<float>(), rstd.data_ptr<float>(), ws.data_ptr<float>(), M, C, (float)mom, (float)eps, relu,
              optr(res), hp ? partials->data_ptr<float>() : nullptr, hp ? (int)partials->size(0) : 0,
              relu ? mask.data_ptr() : nullptr, cur_stream());
    return {y, mean, rstd, mask};
}
Tensor batchnorm_eval(const Tensor& x, const Tensor& w, const Tensor& b, const Tensor& rmean, const Tensor& rvar,
                      double eps, bool relu, const optional<Tensor>& res) {
    check_bn(x, res); GUARD(x);
    Tensor y = at::empty_like(x);
    rn_bn_eval(x.data_ptr(), w.data_ptr(), b.data_ptr(), rmean.data_ptr<float>(), rvar.data_ptr<float>(), y.data_ptr(),
               x.size(0), x.size(1), (float)eps, relu, optr(res), cur_stream());
    return y;
}
// returns (dx, dw, db, g') with g' = dy ⊙ relu'(y) (the fused residual's gradient) when want_gres;
// mask: batchnorm_fwd's relu'(y) bits (read only with relu)
std::tuple<Tensor, Tensor, Tensor, Tensor> batchnorm_bwd(const Tensor& gy, const Tensor& x, const Tensor& mask,
                                                         const Tensor& w, const Tensor& mean, const Tensor& rstd,
                                                         bool relu, bool want_gres, const optional<Tensor>& dw_acc,
                                                         const optional<Tensor>& db_acc) {
    check_bn(gy, c10::nullopt); GUARD(gy);
    const int M = x.size(0), C = x.size(1);
    if (relu)
        TORCH_CHECK(mask.scalar_type() == at::kByte && mask.numel() == (int64_t)M * C / 8 && mask.is_contiguous(),
                    "batchnorm_bwd: relu needs the forward's [M*C/8] uint8 mask");
    Tensor dx = at::empty_like(x);
    // dw_acc / db_acc: gradient views to ADD into (direct accumulation), both or neither
    const bool acc = has(dw_acc);
    TORCH_CHECK(acc == has(db_acc), "batchnorm_bwd: dw_acc and db_acc go together");
    if (acc) {
        for (const Tensor* t : {&*dw_acc, &*db_acc}) {
            CHECK_BF16(*t); CHECK_CONTIG(*t);
            TORCH_CHECK(t->numel() == C && t->device() == x.device(), "batchnorm_bwd: accumulation target shape");
        }
    }
    Tensor dw = acc ? *dw_acc : at::empty({C}, x.options());  // bf16, the parameter dtype
    Tensor db = acc ? *db_acc : at::empty({C}, x.options());
    Tensor gres = want_gres ? at::empty_like(x) : at::empty({0}, x.options());
    Tensor ws = at::empty({rn_bn_ws_floats(M, C)}, x.options().dtype(at::kFloat));
    rn_bn_bwd(gy.data_ptr(), x.data_ptr(), relu ? mask.data_ptr() : nullptr, w.data_ptr(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
              dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr<float>(), M, C, relu,
              want_gres ? gres.data_ptr() : nullptr, acc ? 1 : 0, cur_stream());
    return {dx, dw, db, gres};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(replicann, m) {
    m.def("im2col(Tensor x, int KH, int KW, int S, int P, int Kp) -> Tensor");
    m.def("conv_fwd_implicit(Tensor x, Tensor w, Tensor? bias, int S, int P) -> Tensor");
    m.def("conv_fwd_implicit_stats(Tensor x, Tensor w, Tensor? bias, int S, int P) -> (Tensor, Tensor)");
    m.def("conv_dgrad_implicit(Tensor dy, Tensor w, int H, int W, int P, Tensor(a!)? out=None, bool accumulate=False) -> Tensor");
    m.def("conv_wgrad_implicit(Tensor dy2, Tensor x, int KH, int KW, int S, int P, Tensor(a!)? out=None, "
          "bool accumulate=False) -> Tensor");
    m.def("col2im(Tensor dcols, int N, int H, int W, int C, int KH, int KW, int S, int P, int Kp, Tensor(a!)? out=None, "
          "bool accumulate=False) -> Tensor");
    m.def("maxpool_fwd(Tensor x, int K, int S, int P) -> (Tensor, Tensor)");
    m.def("maxpool_bwd(Tensor gy, Tensor idx, int H, int W, int K, int S, int P) -> Tensor");
    m.def("avgpool_fwd(Tensor x) -> Tensor");
    m.def("avgpool_bwd(Tensor gy, int H, int W) -> Tensor");
    m.def("batchnorm_fwd(Tensor x, Tensor w, Tensor b, Tensor(a!) rmean, Tensor(b!) rvar, float mom, float eps, bool relu, "
          "Tensor? res=None, Tensor? partials=None) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("batchnorm_eval(Tensor x, Tensor w, Tensor b, Tensor rmean, Tensor rvar, float eps, bool relu, "
          "Tensor? res=None) -> Tensor");
    m.def("batchnorm_bwd(Tensor gy, Tensor x, Tensor mask, Tensor w, Tensor mean, Tensor rstd, bool relu, "
          "bool want_gres=False, Tensor(c!)? dw_acc=None, Tensor(d!)? db_acc=None) -> (Tensor, Tensor, Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(replicann, CUDA, m) {
    m.impl("im2col", &im2col);
    m.impl("conv_fwd_implicit", &conv_fwd_implicit);
    m.impl("conv_fwd_implicit_stats", &conv_fwd_implicit_stats);
    m.impl("conv_dgrad_implicit", &conv_dgrad_implicit);
    m.impl("conv_wgrad_implicit", &conv_wgrad_implicit);
    m.impl("col2im", &col2im);
    m.impl("maxpool_fwd", &maxpool_fwd);
    m.impl("maxpool_bwd", &maxpool_bwd);
    m.impl("avgpool_fwd", &avgpool_fwd);
    m.impl("avgpool_bwd", &avgpool_bwd);
    m.impl("batchnorm_fwd", &batchnorm_fwd);
    m.impl("batchnorm_eval", &batchnorm_eval);
    m.impl("batchnorm_bwd", &batchnorm_bwd);
}
