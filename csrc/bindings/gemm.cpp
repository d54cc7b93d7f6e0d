// GEMM bindings: gemm, bias_act_grad, the persistent-GEMM schedule knobs, native_version (kernels:
// gemm_bf16.hip and the units it dispatches to; the autotuner and its table: gemm_tune.cpp).
#include <algorithm>

#include "binding_util.h"
#include "gemm_tune.h"
#include "rn_api.h"

namespace {

// "cfg 7": the vendor library (hipBLASLt through at::mm) for PLAIN GEMMs only (gemm_plan.h: gemm_plain).
// Reachable only by an explicit cfg=7 or, for A/B measurements, REPLICANN_GEMM_LIB=1 (then one more
// autotuner candidate); never a fallback.  Every default-path GEMM runs on the MFMA kernels.
constexpr int kLibCfg = 7;
static void lib_gemm(const Tensor& A, const Tensor& B, bool ta, bool tb, Tensor& c) {
    at::mm_out(c, ta ? A.t() : A, tb ? B.t() : B);
}

static bool capturing() {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(cur_stream(), &cap);
    return cap != hipStreamCaptureStatusNone;
}

// validate → canonicalise the operands → choose (cfg, split) → launch → bias gradient
Tensor gemm(const Tensor& a, const Tensor& b, bool ta, bool tb, const optional<Tensor>& bias,
            const optional<Tensor>& residual, int64_t act, const optional<Tensor>& preact, const optional<Tensor>& out,
            bool accumulate, int64_t split_k, bool out_fp32, const optional<Tensor>& alpha, int64_t cfg,
            const optional<Tensor>& bias_grad) {
    CHECK_CUDA(a); CHECK_BF16(a); CHECK_BF16(b);
    GUARD(a);
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "gemm expects 2-D operands");
    TORCH_CHECK(a.stride(1) == 1 && b.stride(1) == 1, "gemm operands need unit inner stride");
    const int64_t M = ta ? a.size(1) : a.size(0);
    const int64_t K = ta ? a.size(0) : a.size(1);
    const int64_t Kb = tb ? b.size(1) : b.size(0);
    const int64_t N = tb ? b.size(0) : b.size(1);
    TORCH_CHECK(K == Kb, "gemm inner dims differ: ", K, " vs ", Kb);
    Tensor c;
    if (has(out)) {
        c = *out;
        TORCH_CHECK(c.size(0) == M && c.size(1) == N && c.stride(1) == 1, "gemm out shape mismatch");
        out_fp32 = c.scalar_type() == at::kFloat;
    } else {
        c = at::empty({M, N}, a.options().dtype(out_fp32 ? at::kFloat : at::kBFloat16));
    }
    if (has(bias)) { CHECK_BF16(*bias); TORCH_CHECK(bias->numel() == N && bias->is_contiguous()); }
    if (has(residual)) {
        CHECK_BF16(*residual);
        TORCH_CHECK(residual->size(0) == M && residual->size(1) == N && residual->stride(0) == c.stride(0) &&
                    residual->stride(1) == 1, "residual must match the output layout");
    }
    if (has(preact)) {
        CHECK_BF16(*preact);
        TORCH_CHECK(preact->size(0) == M && preact->size(1) == N && preact->stride(0) == c.stride(0));
    }
    // fused activation backward: out = (A·B) ⊙ act'(preact); 6: out = (A·B) ⊙ preact (preact holds gelu'(h),
    // written by the act-5 forward)
    const bool act_bwd = gemm_act_bwd((int)act);
    // bias_grad (act-backward only): Σ_rows of the output accumulated into it — from per-M-tile
    // column partials the epilogue writes (configs that support it), else one reduction pass
    const bool want_bg = has(bias_grad);
    if (want_bg) {
        TORCH_CHECK(act_bwd, "gemm bias_grad needs an activation-backward epilogue");
        CHECK_BF16(*bias_grad);
        TORCH_CHECK(bias_grad->numel() == N && bias_grad->is_contiguous());
        TORCH_CHECK(!out_fp32, "gemm bias_grad needs a bf16 output (both reductions read bf16 rows)");
    }
    // rows: enough for every config (128-row tiles: ceil(M/128); cfg 9: 2 per 256-row tile)
    Tensor colpart = want_bg ? at::empty({2 * ((M + 255) / 256), N}, a.options().dtype(at::kFloat)) : Tensor();
    float* cp = want_bg ? colpart.data_ptr<float>() : nullptr;
    if (act_bwd)
        TORCH_CHECK(!ta && !tb && N % 8 == 0 && has(preact) && !accumulate && !has(bias),
                    "activation-backward epilogue: dgrad layout (A·B, B [K][N]), N % 8 == 0, preact required");
    if (M == 0 || N == 0) return c;

    // K must be a multiple of 8 (16-B rows); pad both operands with zeros otherwise
    Tensor A = a, B = b;
    int64_t Kp = K;
    if (K % 8 != 0) {
        Kp = (K + 7) / 8 * 8;
        A = ta ? at::constant_pad_nd(a, {0, 0, 0, Kp - K}) : at::constant_pad_nd(a, {0, Kp - K});
        B = tb ? at::constant_pad_nd(b, {0, Kp - K}) : at::constant_pad_nd(b, {0, 0, 0, Kp - K});
    }
    if (ta && (M % 8 != 0 || A.stride(0) % 8 != 0)) {  // M-contiguous A needs 16-B aligned rows
        A = A.t().contiguous();
        ta = false;
    }
    if (!tb && (N % 8 != 0 || B.stride(0) % 8 != 0)) {
        B = B.t().contiguous();
        tb = true;
    }
    if (!ta && A.stride(0) % 8 != 0) A = A.contiguous();
    if (tb && B.stride(0) % 8 != 0) B = B.contiguous();
    if (has(alpha)) TORCH_CHECK(alpha->scalar_type() == at::kFloat && alpha->is_cuda());
    // (a one-row operand has no row stride to speak of: a transposed [K][1] made contiguous keeps stride 1)
    const int64_t lda = A.size(0) == 1 ? A.size(1) : A.stride(0), ldb = B.size(0) == 1 ? B.size(1) : B.stride(0);
    const GemmProblem p{M, N, Kp, lda, ldb, c.stride(0), ta, tb, (int)act, out_fp32, accumulate,
                        has(bias), has(residual), has(alpha), has(preact), want_bg, (int)split_k};

    // one launch of this call's operands: the real one, or a tuning trial into scratch
    auto run = [&](const Tensor& o, void* pre, const Tensor& ws, int cfg_, int split_, bool acc, float* colp) {
        return rn_gemm(A.data_ptr(), B.data_ptr(), o.data_ptr(), optr(bias), optr(residual), pre,
                       ws.defined() ? ws.data_ptr<float>() : nullptr, has(alpha) ? alpha->data_ptr<float>() : nullptr,
                       (int)M, (int)N, (int)Kp, p.lda, p.ldb, o.stride(0), ta, tb, (int)act, split_, out_fp32, acc, cfg_,
                       cur_stream(), colp);
    };
    const auto f32 = a.options().dtype(at::kFloat);

    // an explicit cfg or split is taken as given; else the tuning table, else (eager calls only: never
    // while the stream is being captured) a measurement, else the native cost model (cfg / split < 0)
    int icfg = (int)cfg, split = split_k < 0 ? -1 : (int)std::max<int64_t>(1, split_k);
    if (cfg < 0 && split_k <= 0 && !gemm_tune::lookup(p, &icfg, &split) && gemm_tune::enabled() && !capturing()) {
        Tensor scratch = at::empty({M, N}, a.options().dtype(c.scalar_type()));
        // forward activations time WITH their pre-activation / derivative store (a scratch copy): the
        // second output is a large part of the epilogue, and configs differ most in the epilogue
        Tensor scratch_pre = (!act_bwd && act != 0 && has(preact)) ? at::empty({M, N}, a.options()) : Tensor();
        void* pre = act_bwd ? preact->data_ptr() : (scratch_pre.defined() ? scratch_pre.data_ptr() : nullptr);
        Tensor ws = at::empty({rn_gemm_ws_floats(M, N, gemm_tune_splits(p).back())}, f32);
        std::tie(icfg, split) = gemm_tune::tune(p, [&](int cfg_, int split_) {
            if (cfg_ == kLibCfg) { lib_gemm(A, B, ta, tb, scratch); return 0; }
            return run(scratch, pre, ws, cfg_, split_, false, cp);
        });
    }

    if (icfg == kLibCfg) {
        TORCH_CHECK(gemm_plain(p), "gemm cfg 7 (library) is for plain GEMMs only");
        lib_gemm(A, B, ta, tb, c);
        return c;
    }
    // split-K slabs.  split < 0: the native cost model picks (at most 32 slabs, K/split >= 512): size for its worst case
    const int ws_split = split > 1 ? split : (split < 0 ? (int)std::min<int64_t>(32, std::max<int64_t>(1, Kp / 512)) : 1);
    Tensor ws = ws_split > 1 ? at::empty({rn_gemm_ws_floats(M, N, ws_split)}, f32) : Tensor();
    void* pre = has(preact) ? preact->data_ptr() : nullptr;
    auto launch = [&](float* colp) { return run(c, pre, ws, icfg, split, accumulate, colp); };
    int rc = launch(cp);
    if (rc == -3) {  // this config cannot emit column partials: plain GEMM + one reduction pass over C's rows
        rc = launch(nullptr);
        TORCH_CHECK(rc == 0, "rn_gemm rejected shape M=", M, " N=", N, " K=", Kp);
        Tensor part = at::empty({(int64_t)(rn_bias_act_grad_splits((int)M, (int)N) + 32) * N}, f32);
        rn_bias_act_grad(c.data_ptr(), nullptr, c.data_ptr(), nullptr, bias_grad->data_ptr(), part.data_ptr<float>(),
                         (int)M, (int)N, c.stride(0), 0, 1, 1, cur_stream());
        return c;
    }
    TORCH_CHECK(rc == 0, "rn_gemm rejected shape M=", M, " N=", N, " K=", Kp);
    if (want_bg) {
        // as many partial rows as the config that ran wrote: a request (-1, an 11 that falls back) is not one
        const int ran = gemm_resolve(icfg, split, p).cfg;
        Tensor tmp = at::empty({rn_colsum_ws((int)N)}, f32);
        rn_colsum_f32(colpart.data_ptr<float>(), (int)rn_gemm_colpart_rows(ran, (int)M), (int)N, tmp.data_ptr<float>(),
                      bias_grad->data_ptr(), 1, cur_stream());
    }
    return c;
}

// returns (dH, db) with db in bf16 (the parameter dtype)
std::tuple<Tensor, Tensor> bias_act_grad(const Tensor& dy, const optional<Tensor>& h, int64_t act, bool want_bias,
                                         const optional<Tensor>& db_accum) {
    CHECK_CUDA(dy); CHECK_BF16(dy); CHECK_CONTIG(dy);
    GUARD(dy);
    const int M = dy.size(0), N = dy.size(1);
    Tensor dh = act != 0 ? at::empty_like(dy) : dy;
    const bool accum = has(db_accum);
    if (accum) { CHECK_BF16(*db_accum); TORCH_CHECK(db_accum->numel() == N && db_accum->is_contiguous()); }
    Tensor db = accum ? *db_accum : at::empty({want_bias ? N : 0}, dy.options());
    Tensor part = at::empty({want_bias ? (int64_t)(rn_bias_act_grad_splits(M, N) + 32) * N : 1},
                            dy.options().dtype(at::kFloat));
    if (act != 0) { TORCH_CHECK(has(h), "activation grad needs the pre-activation"); CHECK_CONTIG(*h); }
    if (M > 0)
        rn_bias_act_grad(dy.data_ptr(), optr(h), dh.data_ptr(), nullptr, want_bias ? db.data_ptr() : nullptr,
                         part.data_ptr<float>(), M, N, N, (int)act, want_bias, accum, cur_stream());
    else if (want_bias && !accum) db.zero_();
    return {dh, db};
}

// persistent-GEMM schedule knobs (csrc/include/gemm_pk.h: dynamic tile queue, CU reservation)
void gemm_set_sched(int64_t m) { rn_gemm_set_sched((int)m); }
int64_t gemm_get_sched() { return rn_gemm_get_sched(); }
void gemm_set_reserve(int64_t r) { rn_gemm_set_reserve((int)r); }
int64_t gemm_get_reserve() { return rn_gemm_get_reserve(); }
int64_t gemm_sched_init(int64_t dev) { return rn_gemm_sched_init((int)dev); }

int64_t native_version() { return 1; }

}  // namespace

TORCH_LIBRARY_FRAGMENT(replicann, m) {
    m.def("gemm(Tensor a, Tensor b, bool ta=False, bool tb=False, Tensor? bias=None, Tensor? residual=None, int act=0, "
          "Tensor? preact=None, Tensor? out=None, bool accumulate=False, int split_k=0, bool out_fp32=False, "
          "Tensor? alpha=None, int cfg=-1, Tensor(a!)? bias_grad=None) -> Tensor");
    m.def("bias_act_grad(Tensor dy, Tensor? h, int act, bool want_bias, Tensor(a!)? db_accum=None) -> (Tensor, Tensor)");
    m.def("native_version() -> int");
    m.def("gemm_set_sched(int mode) -> ()");
    m.def("gemm_get_sched() -> int");
    m.def("gemm_set_reserve(int cus) -> ()");
    m.def("gemm_get_reserve() -> int");
    m.def("gemm_sched_init(int device) -> int");
}

TORCH_LIBRARY_IMPL(replicann, CUDA, m) {
    m.impl("gemm", &gemm);
    m.impl("bias_act_grad", &bias_act_grad);
}

TORCH_LIBRARY_IMPL(replicann, CompositeExplicitAutograd, m) {
    m.impl("native_version", &native_version);
    m.impl("gemm_set_sched", &gemm_set_sched);
    m.impl("gemm_get_sched", &gemm_get_sched);
    m.impl("gemm_set_reserve", &gemm_set_reserve);
    m.impl("gemm_get_reserve", &gemm_get_reserve);
    m.impl("gemm_sched_init", &gemm_sched_init);
}
