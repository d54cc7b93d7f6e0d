// The streaming attention backward on v_mfma_f32_16x16x32_bf16: the dQ kernel (one workgroup per 64·QG
// queries, loops over keys, also emits −δ) and the dK/dV kernel (one workgroup per 64·KG keys, loops over
// queries), with the launchers that pick an instance.  Included only by the per-head-size instantiation
// units attention_dq_d*.hip / attention_dkdv_d*.hip, so that the family compiles in parallel (as
// gemm_impl.h and gemm_cfg*.hip do); attention.hip's header has the algebra and the LDS layout.
#pragma once

#include "attention_common.h"

namespace rn_attn {
namespace {

// dK, dV: grid (B*H, ceil(Tk/(64·KG))); key group u (< KG) of wave w owns keys
// kb·64·KG + 64·u + 16w + (lane&15).  KG = 2: every Q / dO fragment read from LDS feeds both key
// groups' MFMAs and each wave carries two independent S → P → dS chains (as in the dQ kernel).
template <bool CAUSAL, bool BIAS, bool DROP, int OCC = 3, int KG = 1, int D = 64>
__global__ void __launch_bounds__(256, ((DROP || BIAS) && OCC > 2) ? 2 : OCC) attn_bwd_dkdv64_k(AttnArgs p) {
    constexpr int NS = kNS<D>, NJ = kNJ<D>, TB = kTB<D>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const FragOffT<D> fo = make_fragoff<D>(lane);
    constexpr int KB = 64 * KG;  // keys per block
    // grid (B*H, key blocks): low key blocks see the most queries under causal and, with the block
    // index varying slowest, launch first across ALL heads (longest-first)
    int bh, kb;
    blk_map(p, (p.Tk + KB - 1) / KB, false, bh, kb);  // low key blocks see the most queries: first
    const int b = bh / p.H, h = bh % p.H;
    const int kvw = kb * KB + wave * 16;  // this wave's first key (group 0)
    int kvl[KG];
#pragma unroll
    for (int u = 0; u < KG; ++u) kvl[u] = kvw + 64 * u + c;
    const int off = p.Tk - p.Tq;
    const float sl2 = p.scale * LOG2E;

    const u32x4 qrs = make_rsrc_sgpr(p.q + b * p.q_sb + h * p.q_sh);
    const u32x4 ors = make_rsrc_sgpr(p.dout + b * p.do_sb + h * p.do_sh);
    // per-row softmax statistics ride along with each Q/dO tile (LDS-DMA, 64 floats each)
    const u32x4 lrs = make_rsrc_sgpr(p.lse + ((long)b * p.H + h) * p.Tq, (uint32_t)p.Tq * 4);
    const u32x4 drs = make_rsrc_sgpr(p.delta + ((long)b * p.H + h) * p.Tq, (uint32_t)p.Tq * 4);
    const bf16* kbase = p.k + b * p.k_sb + h * p.k_sh;
    const bf16* vbase = p.v + b * p.v_sb + h * p.v_sh;

    int qt0 = 0;
    if (CAUSAL) qt0 = max(0, (kb * KB - off)) / 64;
    const int nqt = (p.Tq + 63) / 64;
    // buffer i: Q tile [0, TB), dO tile [TB, 2TB), lse [2TB, 2TB + 1K), delta [2TB + 1K, 2TB + 2K)
#define Qt(i) (smem + (i) * (2 * TB + 2048))
#define Ot(i) (smem + TB + (i) * (2 * TB + 2048))
#define Lt(i) (smem + 2 * TB + (i) * (2 * TB + 2048))
#define Dt(i) (smem + 2 * TB + 1024 + (i) * (2 * TB + 2048))
    auto stage = [&](int qt, int buf) {
        stage64_async<D>(qrs, p.q_st, qt * 64, p.Tq, Qt(buf), wave, lane);
        stage64_async<D>(ors, p.do_st, qt * 64, p.Tq, Ot(buf), wave, lane);
        if (wave < 2) {  // lanes 0-15 carry 64 floats; the rest land as zeros past them
            const int r = qt * 64 + lane * 4;
            const uint32_t voff = (lane < 16 && r < p.Tq) ? (uint32_t)(r * 4) : 0xFFFFFFF0u;
            dma16_async(wave == 0 ? lrs : drs, voff, lds_addr(wave == 0 ? Lt(buf) : Dt(buf)));
        }
    };
    if (qt0 < nqt) stage(qt0, 0);

    s16x8 kf[KG][NS], vf[KG][NS];
#pragma unroll
    for (int u = 0; u < KG; ++u) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            kf[u][s] = gload16(kbase + (long)kvl[u] * p.k_st + s * 32 + g * 8, kvl[u] < p.Tk);
            vf[u][s] = gload16(vbase + (long)kvl[u] * p.v_st + s * 32 + g * 8, kvl[u] < p.Tk);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(kf[u][s]), "+v"(vf[u][s]));  // wait here, not in the loop
    }
    f32x4 dvacc[KG][NJ], dkacc[KG][NJ];
#pragma unroll
    for (int u = 0; u < KG; ++u)
#pragma unroll
        for (int jd = 0; jd < NJ; ++jd) { dvacc[u][jd] = (f32x4){0, 0, 0, 0}; dkacc[u][jd] = (f32x4){0, 0, 0, 0}; }

    const float rd = DROP ? 1.f / (1.f - p.p_drop) : 1.f;
    if (p.p_drop > 0.f && p.seed_ptr) p.seed = *p.seed_ptr;
    // Tiles split into masked (causal diagonal of this block's keys, ragged Tq / Tk) and unmasked
    // ones, each class in its own loop: a per-wave `continue` or a runtime mask branch inside one
    // loop makes hipcc carry the accumulators through a phi (a VGPR copy block every tile).
    auto masked_tile = [&](int qt) {
        return (qt * 64 + 64 > p.Tq) || (kb * KB + KB > p.Tk) || (CAUSAL && kb * KB + KB - 1 > qt * 64 + off);
    };
    auto sync_stage = [&](int qt) {
        vm_wait_all();
        __syncthreads();
        if (qt + 1 < nqt) stage(qt + 1, ((qt - qt0) & 1) ^ 1);
    };
    auto body = [&](int qt, auto masked_c, auto buf_c) {  // buf_c: compile-time buffer, see the forward
        constexpr bool MASKED = decltype(masked_c)::value;
        constexpr int cur = decltype(buf_c)::value;
        const int q0 = qt * 64;
        const char* qt_ = Qt(cur);
        const char* ot_ = Ot(cur);
        const float* lt_ = reinterpret_cast<const float*>(Lt(cur));
        const float* dt_ = reinterpret_cast<const float*>(Dt(cur));
        // masked tiles: a (key group u, 16-query fragment qi) block of this wave with no visible
        // (key, query) pair — past Tk / Tq, or wholly above the causal diagonal — skips its MFMAs and
        // VALU (wave-uniform; P = dS = 0 there).  The diagonal's upper blocks and the ragged tail of a
        // T = 197 sequence (ViT) are most of such a tile.
        auto live = [&](int u, int qi) -> bool {
            if constexpr (!MASKED) return true;
            const int k0 = kvw + 64 * u, qa = q0 + qi * 16;
            if (k0 >= p.Tk || qa >= p.Tq) return false;
            return !(CAUSAL && k0 > min(qa + 15, p.Tq - 1) + off);
        };
        f32x4 pq[KG][4], dsq[KG][4];
#pragma unroll
        for (int qi = 0; qi < 4; ++qi) {
            s16x8 af[NS], of[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                af[s] = rowfragx(qt_, qi, s, fo);
                of[s] = rowfragx(ot_, qi, s, fo);
            }
            // lane holds S[q = q0 + 16qi + 4g + r][kv]
            const int ql = qi * 16 + 4 * g;
            const float4 l4 = *reinterpret_cast<const float4*>(lt_ + ql);
            const float4 d4 = *reinterpret_cast<const float4*>(dt_ + ql);
            // the dQ kernel stored −δ: without dropout it is the dP accumulator's start value
            const float ls[4] = {l4.x, l4.y, l4.z, l4.w}, nd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int u = 0; u < KG; ++u) {
                if (MASKED && !live(u, qi)) {
                    pq[u][qi] = (f32x4){0, 0, 0, 0};
                    dsq[u][qi] = (f32x4){0, 0, 0, 0};
                    continue;
                }
                f32x4 sa = {0, 0, 0, 0}, da = {0, 0, 0, 0};
                if constexpr (!DROP) da = (f32x4){nd[0], nd[1], nd[2], nd[3]};
#pragma unroll
                for (int s = 0; s < NS; ++s) sa = MFMA(af[s], kf[u][s], sa, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < NS; ++s) da = MFMA(of[s], vf[u][s], da, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int qg = q0 + ql + r;
                    float x = __builtin_fmaf(sa[r], sl2, -ls[r]);  // lse in base-2 units: one FMA
                    if constexpr (BIAS) {
                        if (qg < p.Tq && kvl[u] < p.Tk)
                            x += p.bias[((long)(p.bias_b > 1 ? b : 0) * p.Tq + qg) * p.Tk + kvl[u]] * LOG2E;
                    }
                    // masked scores: exponent −inf, so P = 0 and dS = 0 follow (one select per element)
                    if constexpr (MASKED)
                        if (kvl[u] >= p.Tk || qg >= p.Tq || (CAUSAL && kvl[u] > qg + off)) x = -INFINITY;
                    float pv = __builtin_amdgcn_exp2f(x);
                    float dpv = da[r];
                    float pd = pv;
                    if constexpr (DROP) {
                        const bool keep = hash_uniform(p.seed, drop_idx(p, b, h, qg, kvl[u])) >= p.p_drop;
                        pd = keep ? pv * rd : 0.f;
                        dpv = keep ? dpv * rd : 0.f;
                    }
                    pq[u][qi][r] = pd;
                    dsq[u][qi][r] = DROP ? pv * (dpv + nd[r]) : pv * dpv;
                }
            }
        }
        // dV^T[d][kv] += dO^T[d][q] Pd[q][kv];  dK^T[d][kv] += Q^T[d][q] dS[q][kv]
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if constexpr (MASKED) {  // both 16-query fragments of this k-step dead for every key group
                bool any = false;
#pragma unroll
                for (int u = 0; u < KG; ++u) any = any || live(u, 2 * ks) || live(u, 2 * ks + 1);
                if (!any) continue;
            }
            s16x8 pb[KG], sb[KG];
#pragma unroll
            for (int u = 0; u < KG; ++u) {
                pb[u] = pack_p(pq[u][2 * ks], pq[u][2 * ks + 1]);
                sb[u] = pack_p(dsq[u][2 * ks], dsq[u][2 * ks + 1]);
            }
#pragma unroll
            for (int jd = 0; jd < NJ; ++jd) {
                const s16x8 ao = colfragx(ot_, ks, jd, fo);
#pragma unroll
                for (int u = 0; u < KG; ++u) dvacc[u][jd] = MFMA(ao, pb[u], dvacc[u][jd], 0, 0, 0);
                const s16x8 aq = colfragx(qt_, ks, jd, fo);
#pragma unroll
                for (int u = 0; u < KG; ++u) dkacc[u][jd] = MFMA(aq, sb[u], dkacc[u][jd], 0, 0, 0);
            }
        }
    };
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    auto step = [&](int qt, auto masked_c, auto buf_c) {
        sync_stage(qt);
        // wave-uniform skip: every query of the tile precedes this wave's first key
        if (decltype(masked_c)::value && CAUSAL && qt * 64 + 63 + off < kvw) return;
        [[clang::always_inline]] body(qt, masked_c, buf_c);
    };
    // tiles [qt, end) with buffer (qt - qt0) & 1 resolved at compile time (always_inline: see dQ)
    auto run = [&](int qt, int end, auto masked_c) {
        if (qt < end && ((qt - qt0) & 1)) [[clang::always_inline]] step(qt++, masked_c, B1{});
        for (; qt + 1 < end; qt += 2) {
            [[clang::always_inline]] step(qt, masked_c, B0{});
            [[clang::always_inline]] step(qt + 1, masked_c, B1{});
        }
        if (qt < end) [[clang::always_inline]] step(qt++, masked_c, B0{});
        return qt;
    };
    int qt = qt0, qe = qt0;
    while (qe < nqt && masked_tile(qe)) ++qe;
    qt = run(qt, qe, std::true_type{});  // diagonal head
    while (qe < nqt && !masked_tile(qe)) ++qe;
    qt = run(qt, qe, std::false_type{});
    run(qt, nqt, std::true_type{});  // ragged tail
#undef Qt
#undef Ot
#undef Lt
#undef Dt
    if (p.bsum) {  // dK / dV column partials for the QKV bias gradient; row = (b, 64-key block)
        const int E = p.H * D, nb64 = (p.Tk + 63) / 64;
#pragma unroll
        for (int u = 0; u < KG; ++u) {
            const int blk = kb * KG + u;
            if (blk < nb64) {  // block-uniform
                float* row = p.bsum + ((long)b * nb64 + blk) * 3 * E + h * D;
                block_colsum64<D>(dkacc[u], p.scale, reinterpret_cast<float*>(smem), row + E, wave, lane);
                block_colsum64<D>(dvacc[u], 1.f, reinterpret_cast<float*>(smem), row + 2 * E, wave, lane);
            }
        }
    }
    float q8m = 0.f;
    const float q8inv = p.q8 ? 1.f / p.q8st[0] : 0.f;
#pragma unroll
    for (int u = 0; u < KG; ++u) {
        if (kvl[u] < p.Tk) {
            const long ko = b * p.dk_sb + (long)kvl[u] * p.dk_st + h * p.dk_sh;
            const long vo = b * p.dv_sb + (long)kvl[u] * p.dv_st + h * p.dv_sh;
            bf16* dkp = p.dk + ko;
            bf16* dvp = p.dv + vo;
#pragma unroll
            for (int jd = 0; jd < NJ; ++jd) {
                const float k0 = dkacc[u][jd][0] * p.scale, k1 = dkacc[u][jd][1] * p.scale,
                            k2 = dkacc[u][jd][2] * p.scale, k3 = dkacc[u][jd][3] * p.scale;
                if (p.q8) {  // (the e5m2 of the bf16-rounded values a separate pass would quantise)
                    attn_q8_store4(p.q8k + ko + jd * 16 + 4 * g, (float)(bf16)k0, (float)(bf16)k1, (float)(bf16)k2,
                                   (float)(bf16)k3, q8inv, q8m);
                    attn_q8_store4(p.q8v + vo + jd * 16 + 4 * g, (float)(bf16)dvacc[u][jd][0], (float)(bf16)dvacc[u][jd][1],
                                   (float)(bf16)dvacc[u][jd][2], (float)(bf16)dvacc[u][jd][3], q8inv, q8m);
                }
                if (!p.q8_only) {
                    bf16x4 k4 = {(bf16)k0, (bf16)k1, (bf16)k2, (bf16)k3};
                    bf16x4 v4 = {(bf16)dvacc[u][jd][0], (bf16)dvacc[u][jd][1], (bf16)dvacc[u][jd][2],
                                 (bf16)dvacc[u][jd][3]};
                    *reinterpret_cast<bf16x4*>(dkp + jd * 16 + 4 * g) = k4;
                    *reinterpret_cast<bf16x4*>(dvp + jd * 16 + 4 * g) = v4;
                }
            }
        }
    }
    if (p.q8) attn_q8_amax(p.q8part2, q8m);
}

// dQ: grid (B*H, ceil(Tq/(64·QG))); query group qg (< QG) of wave w owns queries
// qb·64·QG + 64·qg + 16w + (lane&15).  With QG = 2 every K / V fragment read from LDS feeds
// the MFMAs of two query groups (half the LDS reads per MFMA) and each wave carries two
// independent dependency chains (S → P → dS → dQ) for the scheduler to interleave.
template <bool CAUSAL, bool BIAS, bool DROP, int OCC = 2, int QG = 1, int D = 64>
__global__ void __launch_bounds__(256, OCC) attn_bwd_dq64_k(AttnArgs p) {
    constexpr int NS = kNS<D>, NJ = kNJ<D>, TB = kTB<D>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const FragOffT<D> fo = make_fragoff<D>(lane);
    constexpr int QB = 64 * QG;  // queries per block
    int bh, qb;
    blk_map(p, (p.Tq + QB - 1) / QB, CAUSAL, bh, qb);  // heaviest blocks of every head first
    const int b = bh / p.H, h = bh % p.H;
    const int qw_last = qb * QB + 64 * (QG - 1) + wave * 16;  // this wave's first query of its LAST group
    const int off = p.Tk - p.Tq;
    const float sl2 = p.scale * LOG2E;

    const bf16* qbase = p.q + b * p.q_sb + h * p.q_sh;
    const bf16* dobase = p.dout + b * p.do_sb + h * p.do_sh;
    const u32x4 krs = make_rsrc_sgpr(p.k + b * p.k_sb + h * p.k_sh);
    const u32x4 vrs = make_rsrc_sgpr(p.v + b * p.v_sb + h * p.v_sh);
    int qgl[QG];
    bool qok[QG];
    s16x8 qf[QG][NS], df[QG][NS];
    float lse2[QG], dl[QG];
#pragma unroll
    for (int u = 0; u < QG; ++u) {
        qgl[u] = qb * QB + 64 * u + wave * 16 + c;
        qok[u] = qgl[u] < p.Tq;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            qf[u][s] = gload16(qbase + (long)qgl[u] * p.q_st + s * 32 + g * 8, qok[u]);
            df[u][s] = gload16(dobase + (long)qgl[u] * p.do_st + s * 32 + g * 8, qok[u]);
        }
        lse2[u] = qok[u] ? p.lse[((long)b * p.H + h) * p.Tq + qgl[u]] : INFINITY;  // base-2 units
        // delta = rowsum(dO ∘ O), computed here from the dO fragments already in
        // registers (no separate delta kernel); written out for the dK/dV kernel.
        const bf16* obase = p.o + b * p.o_sb + h * p.o_sh;
        float part = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            s16x8 of = gload16(obase + (long)qgl[u] * p.o_st + s * 32 + g * 8, qok[u]);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                part += (float)__builtin_bit_cast(bf16, (short)of[j]) * (float)__builtin_bit_cast(bf16, (short)df[u][s][j]);
        }
        dl[u] = sum4groups(part);
        // stored NEGATED: the dK/dV kernel starts its dP accumulators at −δ (dP − δ from the MFMA)
        if (qok[u] && g == 0) const_cast<float*>(p.delta)[((long)b * p.H + h) * p.Tq + qgl[u]] = -dl[u];
#pragma unroll
        for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(qf[u][s]), "+v"(df[u][s]));
        asm volatile("" : "+v"(dl[u]));  // loads retired here
    }
    f32x4 dqacc[QG][NJ];
#pragma unroll
    for (int u = 0; u < QG; ++u)
#pragma unroll
        for (int jd = 0; jd < NJ; ++jd) dqacc[u][jd] = (f32x4){0, 0, 0, 0};

    int kv_end = p.Tk;
    if (CAUSAL) kv_end = min(p.Tk, qb * QB + QB + off);
    const int nkv = kv_end > 0 ? (kv_end + 63) / 64 : 0;
#define Kt(i) (smem + (i) * 2 * TB)
#define Vt(i) (smem + TB + (i) * 2 * TB)
    if (nkv > 0) {
        stage64_async<D>(krs, p.k_st, 0, p.Tk, Kt(0), wave, lane);
        stage64_async<D>(vrs, p.v_st, 0, p.Tk, Vt(0), wave, lane);
    }
    const float rd = DROP ? 1.f / (1.f - p.p_drop) : 1.f;
    if (p.p_drop > 0.f && p.seed_ptr) p.seed = *p.seed_ptr;
    // masked (diagonal / ragged) and unmasked tiles in separate loops, see the dK/dV kernel
    auto masked_tile = [&](int t) {
        return (t * 64 + 64 > p.Tk) || (qb * QB + QB > p.Tq) || (CAUSAL && t * 64 + 63 > qb * QB + off);
    };
    auto sync_stage = [&](int t) {
        vm_wait_all();
        __syncthreads();
        if (t + 1 < nkv) {
            stage64_async<D>(krs, p.k_st, (t + 1) * 64, p.Tk, Kt((t & 1) ^ 1), wave, lane);
            stage64_async<D>(vrs, p.v_st, (t + 1) * 64, p.Tk, Vt((t & 1) ^ 1), wave, lane);
        }
    };
    auto body = [&](int t, auto masked_c, auto buf_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
        constexpr int cur = decltype(buf_c)::value;  // compile-time buffer, see the dK/dV kernel
        const int kv0 = t * 64;
        const char* kt = Kt(cur);
        const char* vt = Vt(cur);
        // masked tiles: a (query group u, 16-key block j) of this wave with no visible pair skips
        // its MFMAs and VALU (wave-uniform; dS = 0 there), as in the dK/dV kernel
        auto live = [&](int u, int j) -> bool {
            if constexpr (!MASKED) return true;
            const int qa = qb * QB + 64 * u + wave * 16, k0 = kv0 + 16 * j;
            if (qa >= p.Tq || k0 >= p.Tk) return false;
            return !(CAUSAL && k0 > min(qa + 15, p.Tq - 1) + off);
        };
        f32x4 dsv[QG][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s16x8 kr[NS], vr[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                kr[s] = rowfragx(kt, j, s, fo);
                vr[s] = rowfragx(vt, j, s, fo);
            }
#pragma unroll
            for (int u = 0; u < QG; ++u) {
                if (MASKED && !live(u, j)) {
                    dsv[u][j] = (f32x4){0, 0, 0, 0};
                    continue;
                }
                f32x4 sa = {0, 0, 0, 0}, da = {0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < NS; ++s) sa = MFMA(kr[s], qf[u][s], sa, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < NS; ++s) da = MFMA(vr[s], df[u][s], da, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kvj = kv0 + j * 16 + 4 * g + r;
                    float x = sa[r] * sl2;
                    if constexpr (BIAS) {
                        if (qok[u] && kvj < p.Tk)
                            x += p.bias[((long)(p.bias_b > 1 ? b : 0) * p.Tq + qgl[u]) * p.Tk + kvj] * LOG2E;
                    }
                    float pv = __builtin_amdgcn_exp2f(x - lse2[u]);
                    float dpv = da[r];
                    if constexpr (DROP) {
                        const bool keep = hash_uniform(p.seed, drop_idx(p, b, h, qgl[u], kvj)) >= p.p_drop;
                        dpv = keep ? dpv * rd : 0.f;
                    }
                    dsv[u][j][r] = pv * (dpv - dl[u]);  // (a −δ accumulator start here costs occupancy 3 → 2)
                }
            }
        }
        if constexpr (MASKED) {  // (the dK/dV kernel's −inf-exponent form costs this kernel occupancy 3 → 2)
#pragma unroll
            for (int u = 0; u < QG; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int kvj = kv0 + j * 16 + 4 * g + r;
                        if (kvj >= p.Tk || !qok[u] || (CAUSAL && kvj > qgl[u] + off)) dsv[u][j][r] = 0.f;
                    }
        }
        // dQ^T[d][q] += K^T[d][kv] dS^T[kv][q]
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if constexpr (MASKED) {  // both 16-key blocks of this k-step dead for every query group
                bool any = false;
#pragma unroll
                for (int u = 0; u < QG; ++u) any = any || live(u, 2 * ks) || live(u, 2 * ks + 1);
                if (!any) continue;
            }
            s16x8 sb[QG];
#pragma unroll
            for (int u = 0; u < QG; ++u) sb[u] = pack_p(dsv[u][2 * ks], dsv[u][2 * ks + 1]);
#pragma unroll
            for (int jd = 0; jd < NJ; ++jd) {
                const s16x8 kc = colfragx(kt, ks, jd, fo);
#pragma unroll
                for (int u = 0; u < QG; ++u) dqacc[u][jd] = MFMA(kc, sb[u], dqacc[u][jd], 0, 0, 0);
            }
        }
    };
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    auto step = [&](int t, auto masked_c, auto buf_c) {
        sync_stage(t);
        // wave-uniform skip: every query of this wave (its last group included) precedes the tile
        if (decltype(masked_c)::value && CAUSAL && t * 64 > qw_last + 15 + off) return;
        [[clang::always_inline]] body(t, masked_c, buf_c);
    };
    // (always_inline: with two query groups hipcc otherwise outlines the causal masked step into a
    // real call whose captured state round-trips through scratch)
    auto run = [&](int t, int end, auto masked_c) {
        if (t < end && (t & 1)) [[clang::always_inline]] step(t++, masked_c, B1{});
        for (; t + 1 < end; t += 2) {
            [[clang::always_inline]] step(t, masked_c, B0{});
            [[clang::always_inline]] step(t + 1, masked_c, B1{});
        }
        if (t < end) [[clang::always_inline]] step(t++, masked_c, B0{});
        return t;
    };
    int te = 0;
    while (te < nkv && !masked_tile(te)) ++te;
    const int t = run(0, te, std::false_type{});
    run(t, nkv, std::true_type{});  // diagonal / ragged tail
#undef Kt
#undef Vt
    if (p.bsum) {  // dQ column partials; row = (b, 64-query block) — the dK/dV kernel's row layout
        const int E = p.H * D, nb64 = (p.Tq + 63) / 64;
#pragma unroll
        for (int u = 0; u < QG; ++u) {
            const int blk = qb * QG + u;
            if (blk < nb64) {  // block-uniform
                float* row = p.bsum + ((long)b * nb64 + blk) * 3 * E + h * D;
                block_colsum64<D>(dqacc[u], p.scale, reinterpret_cast<float*>(smem), row, wave, lane);
            }
        }
    }
    float q8m = 0.f;
    const float q8inv = p.q8 ? 1.f / p.q8st[0] : 0.f;
#pragma unroll
    for (int u = 0; u < QG; ++u) {
        if (qok[u]) {
            const long qo = b * p.dq_sb + (long)qgl[u] * p.dq_st + h * p.dq_sh;
            bf16* dqp = p.dq + qo;
#pragma unroll
            for (int jd = 0; jd < NJ; ++jd) {
                bf16x4 q4 = {(bf16)(dqacc[u][jd][0] * p.scale), (bf16)(dqacc[u][jd][1] * p.scale),
                             (bf16)(dqacc[u][jd][2] * p.scale), (bf16)(dqacc[u][jd][3] * p.scale)};
                if (p.q8)
                    attn_q8_store4(p.q8 + qo + jd * 16 + 4 * g, (float)q4[0], (float)q4[1], (float)q4[2], (float)q4[3],
                                   q8inv, q8m);
                if (!p.q8_only) *reinterpret_cast<bf16x4*>(dqp + jd * 16 + 4 * g) = q4;
            }
        }
    }
    if (p.q8) attn_q8_amax(p.q8part, q8m);
}

// D = 64: one group per wave serves bias / dropout only (the plain forms are never built), two groups per
// wave the plain causal / non-causal case; D = 32 / 128: one group for everything.
template <int D>
int launch_dq(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st) {
    if constexpr (D == 64) {
        if (groups == 2) {
            if (a.bias || a.p_drop > 0.f) return ATTN_ERR_PATH;
            const void* k = a.causal ? (const void*)attn_bwd_dq64_k<true, false, false, 2, 2, 64>
                                     : (const void*)attn_bwd_dq64_k<false, false, false, 2, 2, 64>;
            return attn_launch(k, dim3(wgs), 256, 32768, a, st);
        }
    }
    auto kern = [](auto c, auto b, auto d) {
        return (const void*)attn_bwd_dq64_k<decltype(c)::value, decltype(b)::value, decltype(d)::value, 2, 1, D>;
    };
    return groups == 1 ? attn_launch3<D != 64>(kern, a, wgs, 4 * kTB<D>, st) : ATTN_ERR_PATH;
}

template <int D>
int launch_dkdv(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st) {
    constexpr size_t lds = 2 * (2 * kTB<D> + 2048);
    if constexpr (D == 64) {
        if (groups == 2) {
            if (a.bias || a.p_drop > 0.f) return ATTN_ERR_PATH;
            const void* k = a.causal ? (const void*)attn_bwd_dkdv64_k<true, false, false, 2, 2, 64>
                                     : (const void*)attn_bwd_dkdv64_k<false, false, false, 2, 2, 64>;
            return attn_launch(k, dim3(wgs), 256, lds, a, st);
        }
    }
    auto kern = [](auto c, auto b, auto d) {
        return (const void*)attn_bwd_dkdv64_k<decltype(c)::value, decltype(b)::value, decltype(d)::value,
                                              (D == 128 ? 1 : 3), 1, D>;
    };
    return groups == 1 ? attn_launch3<D != 64>(kern, a, wgs, lds, st) : ATTN_ERR_PATH;
}

}  // namespace
}  // namespace rn_attn
