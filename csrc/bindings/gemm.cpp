// GEMM bindings: the measured tile-config autotuner and its tuning table, gemm, bias_act_grad, the
// persistent-GEMM schedule knobs, native_version (kernels: gemm_bf16.hip and the units it dispatches to).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <sstream>
#include <string>

#include "binding_util.h"
#include "rn_api.h"

namespace {

// Measured tile-config / split-K selection.  The first eager call of every GEMM
// shape times the candidate configs on the current stream (into a scratch output;
// the real call then runs once with the winner) and caches the choice.  Calls made
// while the stream is being captured into a hipGraph never tune: they use the
// cache, or the native cost model.  REPLICANN_GEMM_AUTOTUNE=0 disables tuning.
struct TuneKey {
    int64_t M, N, K;
    int ta, tb, act, f32, autosplit, epi;  // epi: bias | residual<<1 | alpha<<2 | accumulate<<3
    bool operator<(const TuneKey& o) const {
        return std::tie(M, N, K, ta, tb, act, f32, autosplit, epi) <
               std::tie(o.M, o.N, o.K, o.ta, o.tb, o.act, o.f32, o.autosplit, o.epi);
    }
};
static std::map<TuneKey, std::pair<int, int>> g_tune;
static std::mutex g_tune_mu;

static bool autotune_enabled() {
    static int v = -1;
    if (v < 0) {
        const char* e = std::getenv("REPLICANN_GEMM_AUTOTUNE");
        v = (e && e[0] == '0') ? 0 : 1;
    }
    return v == 1;
}

std::string gemm_tuning_table() {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    std::ostringstream os;
    os << "[";
    bool first = true;
    for (auto& kv : g_tune) {
        const TuneKey& k = kv.first;
        os << (first ? "" : ",") << "{\"M\":" << k.M << ",\"N\":" << k.N << ",\"K\":" << k.K << ",\"ta\":" << k.ta
           << ",\"tb\":" << k.tb << ",\"act\":" << k.act << ",\"f32\":" << k.f32 << ",\"as\":" << k.autosplit
           << ",\"epi\":" << k.epi << ",\"cfg\":" << kv.second.first << ",\"split\":" << kv.second.second << "}";
        first = false;
    }
    os << "]";
    return os.str();
}

// Replace/insert tuning entries from a gemm_tuning_table() string (data-parallel ranks adopt rank 0's
// measured picks, so every rank runs the same kernels).  Returns the number of entries loaded.
int64_t gemm_tuning_load(const std::string& js) {
    int64_t n = 0;
    size_t pos = 0;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    while ((pos = js.find('{', pos)) != std::string::npos) {
        const size_t end = js.find('}', pos);
        if (end == std::string::npos) break;
        const std::string obj = js.substr(pos, end - pos + 1);
        long M, N, K;
        int ta, tb, act, f32, as, epi, cfg, split;
        if (std::sscanf(obj.c_str(),
                        "{\"M\":%ld,\"N\":%ld,\"K\":%ld,\"ta\":%d,\"tb\":%d,\"act\":%d,\"f32\":%d,\"as\":%d,"
                        "\"epi\":%d,\"cfg\":%d,\"split\":%d}",
                        &M, &N, &K, &ta, &tb, &act, &f32, &as, &epi, &cfg, &split) == 11) {
            g_tune[TuneKey{M, N, K, ta, tb, act, f32, as, epi}] = {cfg, split};
            ++n;
        }
        pos = end + 1;
    }
    return n;
}

// "cfg 7": the vendor library (hipBLASLt through at::mm) for PLAIN GEMMs only — no
// epilogue (bias / activation / residual / accumulate / alpha), bf16 out.  Reachable only
// by an explicit cfg=7 or, for A/B measurements, REPLICANN_GEMM_LIB=1 (then one more
// autotuner candidate); never a fallback.  Every default-path GEMM runs on the MFMA kernels.
constexpr int kLibCfg = 7;
// The library is NOT among the autotuner's candidates unless REPLICANN_GEMM_LIB=1 (A/B runs only).
static bool lib_candidate() {
    static int v = -1;
    if (v < 0) {
        const char* e = std::getenv("REPLICANN_GEMM_LIB");
        v = (e && e[0] == '1') ? 1 : 0;
    }
    return v == 1;
}
static void lib_gemm(const Tensor& A, const Tensor& B, bool ta, bool tb, Tensor& c) {
    at::mm_out(c, ta ? A.t() : A, tb ? B.t() : B);
}

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
    const bool act_bwd = act == 3 || act == 4 || act == 6;
    // bias_grad (act-backward only): Σ_rows of the output accumulated into it — from per-M-tile
    // column partials the epilogue writes (configs that support it), else one reduction pass
    const bool want_bg = has(bias_grad);
    if (want_bg) {
        TORCH_CHECK(act_bwd, "gemm bias_grad needs an activation-backward epilogue");
        CHECK_BF16(*bias_grad);
        TORCH_CHECK(bias_grad->numel() == N && bias_grad->is_contiguous());
    }
    // rows: enough for every config (128-row tiles: ceil(M/128); cfg 9: 2 per 256-row tile)
    Tensor colpart = want_bg ? at::empty({2 * ((M + 255) / 256), N}, a.options().dtype(at::kFloat)) : Tensor();
    float* cp = want_bg ? colpart.data_ptr<float>() : nullptr;
    if (act_bwd)
        TORCH_CHECK(!ta && !tb && N % 8 == 0 && has(preact) && !accumulate && !has(bias),
                    "activation-backward epilogue: dgrad layout (A·B, B [K][N]), N % 8 == 0, preact required");
    if (M == 0 || N == 0) return c;
    int split = split_k < 0 ? -1 : (int)std::max<int64_t>(1, split_k);
    Tensor ws;  // split-K slabs: allocated once the split is known (tuned / cached / explicit)
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
    if (c.stride(0) % 4 != 0 && (bias || residual)) { /* epilogue handles unaligned via scalar path */ }
    if (has(alpha)) TORCH_CHECK(alpha->scalar_type() == at::kFloat && alpha->is_cuda());
    if (cfg < 0 && split_k <= 0) {
        const int epi = (has(bias) ? 1 : 0) | (has(residual) ? 2 : 0) | (has(alpha) ? 4 : 0) | (accumulate ? 8 : 0) |
                        (want_bg ? 16 : 0);
        const TuneKey key{M, N, Kp, (int)ta, (int)tb, (int)act, (int)out_fp32, split_k < 0 ? 1 : 0, epi};
        bool hit = false;
        {
            std::lock_guard<std::mutex> lk(g_tune_mu);
            auto it = g_tune.find(key);
            if (it != g_tune.end()) { cfg = it->second.first; split = it->second.second; hit = true; }
        }
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(cur_stream(), &cap);
        if (!hit && autotune_enabled() && cap == hipStreamCaptureStatusNone) {
            Tensor scratch = at::empty({M, N}, a.options().dtype(out_fp32 ? at::kFloat : at::kBFloat16));
            // forward activations time WITH their pre-activation / derivative store (a scratch copy): the
            // second output is a large part of the epilogue, and configs differ most in the epilogue
            const bool act_fwd_pre = !act_bwd && act != 0 && has(preact);
            Tensor scratch_pre = act_fwd_pre ? at::empty({M, N}, a.options()) : Tensor();
            const bool plain = !has(bias) && !has(residual) && act == 0 && !has(alpha) && !out_fp32 && !accumulate &&
                               c.is_contiguous();
            // decode-size GEMMs (M <= 64 rows, x·Wᵀ): the skinny config 10 joins the candidates
            const bool skinny = M <= 64 && !ta && tb && !act_bwd && !accumulate && !want_bg;
            int cfgs[9] = {9, 1, 6, 0, 2, 8, 0, 0, 0};
            int ncfg = 6;
            // the one-wave-per-SIMD persistent kernel (gemm_w1.h): A K-contiguous, plain / bias / alpha epilogue
            const bool w1_ok = !ta && act == 0 && !has(residual) && !accumulate && !out_fp32 &&
                               !want_bg && Kp % 64 == 0 && Kp >= 128 && N % 8 == 0 && c.stride(0) % 8 == 0 &&
                               !(has(bias) && has(alpha));
            if (w1_ok) cfgs[ncfg++] = 11;
            if (plain && lib_candidate()) cfgs[ncfg++] = kLibCfg;
            if (skinny) cfgs[ncfg++] = 10;
            // non-powers of two too: the split that makes tiles × split just fill the 256 CUs
            // (e.g. 48 tiles × 5 = 240) beats the next power of two by up to 25 %
            // up to 128 slabs for tiny outputs over a huge K (e.g. a conv-stem weight gradient: 64×147
            // outputs, 3 M pixels), where even 16 splits leave most CUs idle
            // (7 and 14: 36 output tiles of 256² — GPT-2's 3072×768 weight gradients — × 7 = 252 WGs)
            const int splits[16] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 24, 32, 64, 128};
            const long out_tiles = ((M + 255) / 256) * ((N + 255) / 256);
            const int nsplit = split_k < 0 ? (out_tiles * 16 < 256 ? 16 : 12) : 1;
            Tensor tws = at::empty({rn_gemm_ws_floats(M, N, splits[nsplit - 1])}, a.options().dtype(at::kFloat));
            hipEvent_t e0, e1;
            (void)hipEventCreate(&e0);
            (void)hipEventCreate(&e1);
            float best_ms = 1e30f;
            int best_cfg = 0, best_split = 1;
            // two interleaved rounds over all candidates, best-of per candidate: one round's
            // clock / cache transients otherwise flip close calls (e.g. library vs MFMA kernel)
            for (int round = 0; round < 2; ++round)
            for (int ci = 0; ci < ncfg; ++ci) {
                for (int si = 0; si < nsplit; ++si) {
                    const int sp = splits[si];
                    if (sp > 1 && Kp / sp < 256) break;
                    if (cfgs[ci] == kLibCfg && sp > 1) break;
                    if (cfgs[ci] == 11 && sp > 1) break;  // (no split-K form)
                    auto run = [&]() {
                        if (cfgs[ci] == kLibCfg) { lib_gemm(A, B, ta, tb, scratch); return 0; }
                        return rn_gemm(A.data_ptr(), B.data_ptr(), scratch.data_ptr(), optr(bias), optr(residual),
                                       act_bwd ? preact->data_ptr() : (act_fwd_pre ? scratch_pre.data_ptr() : nullptr),
                                       tws.data_ptr<float>(), has(alpha) ? alpha->data_ptr<float>() : nullptr,
                                       (int)M, (int)N, (int)Kp, A.stride(0), B.stride(0), scratch.stride(0), ta, tb, (int)act,
                                       sp, out_fp32, 0, cfgs[ci], cur_stream(), cp);
                    };
                    if (run() != 0) continue;
                    (void)hipEventRecord(e0, cur_stream());
                    for (int r = 0; r < 5; ++r) run();
                    (void)hipEventRecord(e1, cur_stream());
                    (void)hipEventSynchronize(e1);
                    float ms = 0.f;
                    (void)hipEventElapsedTime(&ms, e0, e1);
                    if (ms < best_ms) { best_ms = ms; best_cfg = cfgs[ci]; best_split = sp; }
                }
            }
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            {
                std::lock_guard<std::mutex> lk(g_tune_mu);
                g_tune[key] = {best_cfg, best_split};
            }
            if (std::getenv("REPLICANN_GEMM_VERBOSE"))
                std::fprintf(stderr, "[replicann gemm tune] M=%ld N=%ld K=%ld ta=%d tb=%d act=%ld -> cfg %d split %d (%.3f ms)\n",
                             (long)M, (long)N, (long)Kp, (int)ta, (int)tb, (long)act, best_cfg, best_split, best_ms / 5);
            cfg = best_cfg;
            split = best_split;
        }
    }
    if (cfg == kLibCfg) {
        TORCH_CHECK(!has(bias) && !has(residual) && act == 0 && !has(alpha) && !out_fp32 && !accumulate,
                    "gemm cfg 7 (library) is for plain GEMMs only");
        lib_gemm(A, B, ta, tb, c);
        return c;
    }
    // split < 0: the native cost model picks (at most 32 slabs, K/split >= 512): size for its worst case
    const int ws_split = split > 1 ? split : (split < 0 ? (int)std::min<int64_t>(32, std::max<int64_t>(1, Kp / 512)) : 1);
    if (ws_split > 1) ws = at::empty({rn_gemm_ws_floats(M, N, ws_split)}, a.options().dtype(at::kFloat));
    auto launch = [&](float* colp) {
        return rn_gemm(A.data_ptr(), B.data_ptr(), c.data_ptr(), optr(bias), optr(residual),
                       has(preact) ? preact->data_ptr() : nullptr,
                       ws.defined() ? ws.data_ptr<float>() : nullptr,
                       has(alpha) ? alpha->data_ptr<float>() : nullptr, (int)M, (int)N, (int)Kp,
                       A.stride(0), B.stride(0), c.stride(0), ta, tb, (int)act, split, out_fp32, accumulate, (int)cfg,
                       cur_stream(), colp);
    };
    int rc = launch(cp);
    if (rc == -3) {  // this config cannot emit column partials: plain GEMM + one reduction pass over C
        rc = launch(nullptr);
        TORCH_CHECK(rc == 0, "rn_gemm rejected shape M=", M, " N=", N, " K=", Kp);
        Tensor part = at::empty({(int64_t)(rn_bias_act_grad_splits((int)M, (int)N) + 32) * N}, a.options().dtype(at::kFloat));
        rn_bias_act_grad(c.data_ptr(), nullptr, c.data_ptr(), nullptr, bias_grad->data_ptr(), part.data_ptr<float>(),
                         (int)M, (int)N, 0, 1, 1, cur_stream());
        return c;
    }
    TORCH_CHECK(rc == 0, "rn_gemm rejected shape M=", M, " N=", N, " K=", Kp);
    if (want_bg) {
        Tensor tmp = at::empty({rn_colsum_ws((int)N)}, a.options().dtype(at::kFloat));
        rn_colsum_f32(colpart.data_ptr<float>(), (int)rn_gemm_colpart_rows((int)cfg, (int)M), (int)N, tmp.data_ptr<float>(),
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
                         part.data_ptr<float>(), M, N, (int)act, want_bias, accum, cur_stream());
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
    m.def("gemm(Tensor a, Tensor b, bool ta, bool tb, Tensor? bias, Tensor? residual, int act, Tensor? preact, "
          "Tensor? out, bool accumulate, int split_k, bool out_fp32, Tensor? alpha=None, int cfg=-1, "
          "Tensor(a!)? bias_grad=None) -> Tensor");
    m.def("bias_act_grad(Tensor dy, Tensor? h, int act, bool want_bias, Tensor(a!)? db_accum=None) -> (Tensor, Tensor)");
    m.def("native_version() -> int");
    m.def("gemm_tuning_table() -> str");
    m.def("gemm_tuning_load(str table) -> int");
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
    m.impl("gemm_tuning_table", &gemm_tuning_table);
    m.impl("gemm_tuning_load", &gemm_tuning_load);
}
