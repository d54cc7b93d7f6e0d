// The bf16 GEMM's measured tile-config / split-K selection: the tuning table, its text form, and tune().
// The first eager call of every GEMM problem times the candidates gemm_plan.h lists for it on the current
// stream (into a scratch output; the real call then runs once with the winner) and caches the choice.
// Calls made while the stream is being captured into a hipGraph never tune: they use the cache, or the
// native cost model.  REPLICANN_GEMM_AUTOTUNE=0 disables tuning.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <sstream>
#include <string>

#include "binding_util.h"
#include "gemm_tune.h"

namespace {

// M, N, K, ta, tb, act, f32 (output), as (split left to the tuner), epi (GemmProblem::epi())
using TuneKey = std::tuple<int64_t, int64_t, int64_t, int, int, int, int, int, int>;
static std::map<TuneKey, std::pair<int, int>> g_tune;
static std::mutex g_tune_mu;

TuneKey key_of(const GemmProblem& p) {
    return {p.M, p.N, p.K, (int)p.ta, (int)p.tb, p.act, (int)p.out_f32, p.split_req < 0 ? 1 : 0, p.epi()};
}

bool env_is(const char* name, char c) {
    const char* e = std::getenv(name);
    return e && e[0] == c;
}

std::string gemm_tuning_table() {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    std::ostringstream os;
    os << "[";
    bool first = true;
    for (auto& kv : g_tune) {
        const auto& [M, N, K, ta, tb, act, f32, as, epi] = kv.first;
        os << (first ? "" : ",") << "{\"M\":" << M << ",\"N\":" << N << ",\"K\":" << K << ",\"ta\":" << ta
           << ",\"tb\":" << tb << ",\"act\":" << act << ",\"f32\":" << f32 << ",\"as\":" << as
           << ",\"epi\":" << epi << ",\"cfg\":" << kv.second.first << ",\"split\":" << kv.second.second << "}";
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

// Debug: the flattened (cfg, split) pairs tune() would time for a problem whose operands are already
// canonical (K % 8 == 0, contiguous A and B).  No tensors: runs on a host without a GPU.
std::vector<int64_t> gemm_candidates_op(int64_t M, int64_t N, int64_t K, bool ta, bool tb, int64_t act, bool out_fp32,
                                        bool accumulate, int64_t split_k, bool bias, bool residual, bool alpha,
                                        bool bias_grad, int64_t ldc) {
    const GemmProblem p{M, N, K, ta ? M : K, tb ? K : N, ldc, ta, tb, (int)act, out_fp32, accumulate,
                        bias, residual, alpha, /*preact=*/act != 0, bias_grad, (int)split_k};
    std::vector<int64_t> flat;
    for (const auto& c : gemm_candidates(p, gemm_tune::lib_candidate())) {
        flat.push_back(c.first);
        flat.push_back(c.second);
    }
    return flat;
}

}  // namespace

namespace gemm_tune {

bool enabled() {
    static const bool v = !env_is("REPLICANN_GEMM_AUTOTUNE", '0');
    return v;
}
bool lib_candidate() {
    static const bool v = env_is("REPLICANN_GEMM_LIB", '1');
    return v;
}

bool lookup(const GemmProblem& p, int* cfg, int* split) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    const auto it = g_tune.find(key_of(p));
    if (it == g_tune.end()) return false;
    *cfg = it->second.first;
    *split = it->second.second;
    return true;
}

std::pair<int, int> tune(const GemmProblem& p, const Trial& trial) {
    struct Event {
        hipEvent_t e;
        Event() { (void)hipEventCreate(&e); }
        ~Event() { (void)hipEventDestroy(e); }
    } e0, e1;
    float best_ms = 1e30f;
    std::pair<int, int> best{0, 1};
    // two interleaved rounds over all candidates, best-of per candidate: one round's
    // clock / cache transients otherwise flip close calls (e.g. library vs MFMA kernel)
    for (int round = 0; round < 2; ++round)
        for (const auto& c : gemm_candidates(p, lib_candidate())) {
            TORCH_CHECK(trial(c.first, c.second) == 0, "gemm tune: rn_gemm rejected cfg ", c.first, " split ", c.second,
                        ", which gemm_plan.h lists for M=", p.M, " N=", p.N, " K=", p.K);
            (void)hipEventRecord(e0.e, cur_stream());
            for (int r = 0; r < 5; ++r) trial(c.first, c.second);
            (void)hipEventRecord(e1.e, cur_stream());
            (void)hipEventSynchronize(e1.e);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0.e, e1.e);
            if (ms < best_ms) { best_ms = ms; best = c; }
        }
    {
        std::lock_guard<std::mutex> lk(g_tune_mu);
        g_tune[key_of(p)] = best;
    }
    if (std::getenv("REPLICANN_GEMM_VERBOSE"))
        std::fprintf(stderr, "[replicann gemm tune] M=%ld N=%ld K=%ld ta=%d tb=%d act=%ld -> cfg %d split %d (%.3f ms)\n",
                     p.M, p.N, p.K, (int)p.ta, (int)p.tb, (long)p.act, best.first, best.second, best_ms / 5);
    return best;
}

}  // namespace gemm_tune

TORCH_LIBRARY_FRAGMENT(replicann, m) {
    m.def("gemm_tuning_table() -> str");
    m.def("gemm_tuning_load(str table) -> int");
    m.def("gemm_candidates(int M, int N, int K, bool ta, bool tb, int act, bool out_fp32, bool accumulate, int split_k, "
          "bool bias, bool residual, bool alpha, bool bias_grad, int ldc) -> int[]");
}

TORCH_LIBRARY_IMPL(replicann, CompositeExplicitAutograd, m) {
    m.impl("gemm_tuning_table", &gemm_tuning_table);
    m.impl("gemm_tuning_load", &gemm_tuning_load);
    m.impl("gemm_candidates", &gemm_candidates_op);
}
