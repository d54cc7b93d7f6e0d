// The host-side plan of a bf16 GEMM: the canonical problem, the one statement of which tile config takes
// which problem, and the ordered candidates the autotuner times.  Read by rn_gemm and the launchers it
// forwards to (csrc/kernels/gemm_bf16.hip, gemm_skinny.hip), by the bindings (csrc/bindings/gemm.cpp,
// gemm_tune.cpp) and, through the debug op gemm_candidates, by tests on hosts without a GPU.
// Plain C++17: no torch, no HIP.  All sizes and strides are in elements.
#pragma once
#include <utility>
#include <vector>

// activation codes (ACT_* of common.h; gemm_bf16.hip asserts the two agree)
constexpr bool gemm_act_bwd(int act) { return act == 3 || act == 4 || act == 6; }
constexpr bool gemm_act_skinny(int act) { return act == 0 || act == 1 || act == 2 || act == 5; }

// The problem after the binding's K padding and forced transposes, as rn_gemm receives it.
struct GemmProblem {
    long M, N, K;        // K a multiple of 8
    long lda, ldb, ldc;  // row strides
    bool ta, tb;         // rn_gemm's trans_a / trans_b
    int act;
    bool out_f32, accumulate;
    bool bias, residual, alpha, preact, colpart;  // operands given (colpart: the fused bias gradient)
    int split_req;                                // the caller's split_k: < 0 auto, 0 / 1 none, > 1 explicit
    // the epilogue bits of the tuning key
    int epi() const { return (bias ? 1 : 0) | (residual ? 2 : 0) | (alpha ? 4 : 0) | (accumulate ? 8 : 0) | (colpart ? 16 : 0); }
};

// Tile configs (the list above rn_gemm says what each one is).  bm: tile rows, the unit of the column-partial
// matrix; colpart: the epilogue can emit per-M-tile column sums (256x192, CPR 24, and the simple 256-wide
// configs are not wired for it); splitk: has a split-K form.  An id that is not listed runs cfg 0's kernel
// and is described as rn_gemm_cfg_bm always has: 256 rows.
struct GemmCfg { int id, bm; bool colpart, splitk; };
constexpr GemmCfg kGemmCfgs[] = {
    {0, 128, true, true},  {1, 256, true, true},  {2, 256, true, true},    {3, 128, false, true},
    {4, 256, false, true}, {5, 128, true, true},  {6, 256, false, true},   {7, 256, false, false},
    {8, 256, true, true},  {9, 128, true, true},  {10, 256, false, true},  {11, 256, false, false}};
constexpr GemmCfg gemm_cfg(int id) {
    for (const GemmCfg& c : kGemmCfgs)
        if (c.id == id) return c;
    return {id, 256, true, true};
}
// rows of the column-partial matrix a config writes (cfg 9: one row per (256-row tile, wave row))
inline long gemm_colpart_rows(int cfg, long M) {
    return cfg == 9 ? 2 * ((M + 255) / 256) : (M + gemm_cfg(cfg).bm - 1) / gemm_cfg(cfg).bm;
}

// split-K slabs are whole 64-deep K tiles: the depth of a slab and the number of slabs a requested split becomes
inline int gemm_k_per_split(long K, int split) {
    const int s = split < 1 ? 1 : split;
    return (int)(((K + s - 1) / s + 63) / 64 * 64);
}
inline int gemm_slabs(long K, int split) { return (int)((K + gemm_k_per_split(K, split) - 1) / gemm_k_per_split(K, split)); }

// What every config needs of the operands (rn_gemm's -1): 16-byte rows, and the fused activation
// backward in the dgrad layout (A·B, B [K][N]) with its saved pre-activation.
inline bool gemm_operands_ok(const GemmProblem& p) {
    if (p.K % 8 != 0 || p.lda % 8 != 0 || p.ldb % 8 != 0) return false;
    if (p.ta && p.M % 8 != 0) return false;   // an M-contiguous A
    if (!p.tb && p.N % 8 != 0) return false;  // an N-contiguous B
    return !(gemm_act_bwd(p.act) && (p.ta || p.tb || !p.preact));
}
// Can `cfg` emit the column partials of p's fused bias gradient (rn_gemm's -3 when not)?  The tuner times
// into a contiguous scratch output (ldc = N), so it never sees the ldc rule; the launch into the real
// output does, and the binding then reduces C itself.
inline bool gemm_colpart_ok(int cfg, const GemmProblem& p, int split, bool for_tuner = false) {
    return gemm_cfg(cfg).colpart && gemm_act_bwd(p.act) && gemm_slabs(p.K, split) <= 1 && !p.out_f32 && p.N % 8 == 0 &&
           (for_tuner || p.ldc % 8 == 0);
}
// cfg 9's own kernel (gemm_pk.h); a problem it does not take runs cfg 1's kernel under the id 9
inline bool gemm_pk_ok(const GemmProblem& p) { return p.N % 8 == 0 && p.ldc % 8 == 0 && !(p.out_f32 && p.act != 0); }
// no epilogue at all, bf16 out: what the vendor library (cfg 7) is for
inline bool gemm_plain(const GemmProblem& p) {
    return !p.bias && !p.residual && p.act == 0 && !p.alpha && !p.out_f32 && !p.accumulate;
}

// Does config `cfg` take problem p with `split` (<= 1: none)?  The only statement of each config's contract.
// for_tuner: as a candidate of the autotuner, which is stricter in two places where the explicit path is not:
//   * cfg 11 with a residual: the launcher has residual bodies (x·Wᵀ, no alpha, >= 6 K tiles) and an
//     explicit cfg=11 uses them, but the tuner has never offered cfg 11 to a problem with a residual;
//   * cfg 7 as a candidate wants a contiguous output, an explicit cfg=7 writes any row stride.
// A false answer means different things to rn_gemm: cfg 11 falls back to 9, cfg 10 and the operand rules
// return -1, column partials return -3.
inline bool gemm_cfg_takes(int cfg, const GemmProblem& p, int split, bool for_tuner = false) {
    if (!gemm_operands_ok(p)) return false;
    if (p.colpart && !gemm_colpart_ok(cfg, p, split, for_tuner)) return false;
    if (split > 1 && !gemm_cfg(cfg).splitk) return false;
    switch (cfg) {
        case 7: return gemm_plain(p) && (!for_tuner || p.ldc == p.N);
        case 10:  // skinny-M decode GEMM: the Linear forward layout, at most 64 rows
            return p.M >= 1 && p.M <= 64 && !p.ta && p.tb && !p.accumulate && gemm_act_skinny(p.act);
        case 11:  // one wave per SIMD: A K-contiguous, whole 64-deep K tiles (>= 2), plain / bias / alpha epilogue
            return !p.ta && p.act == 0 && !p.accumulate && !p.out_f32 && p.K % 64 == 0 && p.K >= 128 && p.N % 8 == 0 &&
                   p.ldc % 8 == 0 && !(p.bias && p.alpha) &&
                   (!p.residual || (!for_tuner && p.tb && !p.alpha && p.K / 64 >= 6));
        default: return true;  // the tile configs take every epilogue (9: see gemm_pk_ok)
    }
}

// The native chooser behind cfg / split < 0: a wave-quantisation cost model calibrated on MI355X
// measurements of these kernels (scripts/microbench.py).  A 128² block runs 2 per CU, a 256² block 1 per
// CU and ~13 % faster per FLOP (half the L2→LDS bytes per FLOP); a launch takes ceil(tiles / resident
// slots) rounds.
struct GemmChoice { int cfg, split; };
inline GemmChoice gemm_pick(long M, long N, long K, int split_req) {
    auto ntiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
    const double flop_s_cu = 2.9e12;  // effective per-CU bf16 rate of the 128² config
    // candidates: cfg id, BM, BN, resident blocks (slots), relative per-CU rate
    const int cid[4] = {0, 1, 6, 2};
    const int bm[4] = {128, 256, 256, 256}, bn[4] = {128, 256, 192, 128}, slots[4] = {512, 256, 256, 256};
    const double rate[4] = {1.0, 1.16, 1.0, 0.9};
    GemmChoice best = {0, 1};
    double best_t = 1e30;
    for (int c = 0; c < 4; ++c) {
        for (int sp = 1; sp <= 32; sp *= 2) {
            if (split_req > 0 && sp != split_req) continue;
            if (split_req <= 0 && sp > 1 && K / sp < 512) break;
            // split-K only when the unsplit grid cannot fill the resident slots
            if (split_req <= 0 && sp > 1 && ntiles(bm[c], bn[c]) >= slots[c]) break;
            const long kps = ((K + sp - 1) / sp + 63) / 64 * 64;
            const long tiles = ntiles(bm[c], bn[c]) * sp;
            const long rounds = (tiles + slots[c] - 1) / slots[c];
            const double per_block = 2.0 * bm[c] * bn[c] * kps / (flop_s_cu * rate[c]) * (c == 0 ? 2.0 : 1.0);
            double t = rounds * per_block + 2.5e-6;  // + prologue/epilogue per launch
            if (sp > 1) t += ((double)M * N * (4.0 * sp + 2.0)) / 4.0e12 + 3e-6;
            if (t < best_t * 0.98) { best_t = t; best = {cid[c], sp}; }
        }
    }
    return best;
}

// The (cfg, split) that runs for a requested pair: the one place a request is resolved.  rn_gemm launches
// what this returns, and the binding sizes the column-partial reduction from it (gemm_colpart_rows of the
// REQUESTED id is wrong whenever the two differ: -1 and an 11 that falls back both run cfg 9, which writes
// two partial rows per 256-row tile).  cfg 10 has its own launcher and stays; cfg 11 stays where it takes
// the problem (if its launcher still declines, rn_gemm runs cfg 9: never with column partials, which
// cfg 11 does not take); an id that is not in the table runs cfg 0's kernel.
inline GemmChoice gemm_resolve(int cfg, int split, const GemmProblem& p) {
    if (cfg == 10) return {cfg, split};
    if (cfg == 11) {
        if (gemm_cfg_takes(11, p, split)) return {cfg, split};
        cfg = 9;
    }
    if (cfg < 0 || split < 0) {
        const GemmChoice ch = gemm_pick(p.M, p.N, p.K, split);
        if (cfg < 0) cfg = gemm_pk_ok(p) ? 9 : ch.cfg;
        if (split < 0) split = ch.split;
    }
    if (cfg == 9 && !gemm_pk_ok(p)) cfg = 1;  // shapes the persistent kernel does not take
    if (cfg >= 90 && cfg < 90 + 256) return {cfg, split};  // development-only ablation builds of cfg 9
    if (cfg == 7 || cfg > 11) cfg = 0;  // not a kernel of rn_gemm's
    return {cfg, split};
}

// The split-K values the tuner tries, before a config's own limits.  Non-powers of two too: the split that
// makes tiles × split just fill the 256 CUs (48 tiles × 5 = 240; 36 tiles of 256², GPT-2's 3072×768 weight
// gradients, × 7 = 252) beats the next power of two by up to 25 %.  Up to 128 slabs only for tiny outputs
// over a huge K (a conv-stem weight gradient: 64×147 outputs, 3 M pixels), where even 16 leave most CUs idle.
inline std::vector<int> gemm_tune_splits(const GemmProblem& p) {
    static const int splits[16] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 24, 32, 64, 128};
    const long out_tiles = ((p.M + 255) / 256) * ((p.N + 255) / 256);
    const int n = p.split_req < 0 ? (out_tiles * 16 < 256 ? 16 : 12) : 1;
    return std::vector<int>(splits, splits + n);
}
// The (cfg, split) pairs the autotuner times for p, in its order; the first strictly fastest one wins.
// Aliases stay: cfg 9 on a problem gemm_pk_ok rejects times cfg 1's kernel twice, and tables hold such 9s.
inline std::vector<std::pair<int, int>> gemm_candidates(const GemmProblem& p, bool lib_enabled) {
    std::vector<std::pair<int, int>> out;
    const std::vector<int> splits = gemm_tune_splits(p);
    for (int cfg : {9, 1, 6, 0, 2, 8, 11, 7, 10}) {
        if (cfg == 7 && !lib_enabled) continue;
        for (int sp : splits) {
            if (sp > 1 && p.K / sp < 256) break;
            if (gemm_cfg_takes(cfg, p, sp, true)) out.emplace_back(cfg, sp);
        }
    }
    return out;
}
