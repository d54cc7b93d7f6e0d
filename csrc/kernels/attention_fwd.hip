// Attention forward on v_mfma_f32_16x16x32_bf16 (the algebra and LDS layout: attention.hip's header):
// the single-loop attn_fwd64_k (D = 32 / 128 for everything, D = 64 with an additive bias or dropout) and
// the split-loop attn_fwd64v2_k (D = 64 non-causal without either, Tq or Tk above RES_T).
#include "attention_common.h"

namespace rn_attn {
namespace {

// row fragment: 8 bf16 of row `row`, columns 32*s + 8*(lane>>4) .. +7
template <int D = 64>
RN_DEV s16x8 rowfrag(const char* t, int row, int s, int lane) {
    const int chunk = s * 4 + (lane >> 4);
    return *reinterpret_cast<const s16x8*>(t + row * kRB<D> + ((chunk ^ swz<D>(row)) << 4));
}

// column fragment: column c0 + (lane&15), rows {rb + 4g + 0..3} ∪ {rb + 16 + 4g + 0..3}
template <int D = 64>
RN_DEV s16x8 colfrag(const char* t, int rb, int c0, int lane) {
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, p = i & 3;
    const int ch = (c0 >> 3) + (p >> 1);
    const int r0 = rb + 4 * g + qq, r1 = r0 + 16;
    const char* a0 = t + r0 * kRB<D> + ((ch ^ swz<D>(r0)) << 4) + (p & 1) * 8;
    const char* a1 = t + r1 * kRB<D> + ((ch ^ swz<D>(r1)) << 4) + (p & 1) * 8;
    s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a1);
    s16x8 r;
    r[0] = v0[0]; r[1] = v0[1]; r[2] = v0[2]; r[3] = v0[3];
    r[4] = v1[0]; r[5] = v1[1]; r[6] = v1[2]; r[7] = v1[3];
    return r;
}

// D = 32 / 64 / 128 (template); at D = 64 the default for bias / dropout, D = 32 / 128 for everything.
// QI: 16-query fragments per wave (block = 64·QI queries); 1 at D = 128 to fit the O accumulators.
// The bias / dropout variants run at occupancy ≤ 2: the per-score loads / hash need the registers.
template <bool CAUSAL, bool BIAS, bool DROP, int D = 64, int OCC = 3, int QI = 2>
__global__ void __launch_bounds__(256, ((DROP || BIAS) && OCC > 2) ? 2 : OCC) attn_fwd64_k(AttnArgs p) {
    constexpr int NS = kNS<D>, NJ = kNJ<D>, TB = kTB<D>, QBLK = 64 * QI;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // grid (B*H, blocks): the block index varies SLOWEST, so under causal masking every head's
    // heaviest query block is dispatched before any lighter one (longest-first over the grid)
    int bh, qb;
    blk_map(p, (p.Tq + QBLK - 1) / QBLK, CAUSAL, bh, qb);
    const int b = bh / p.H, h = bh % p.H;
    const int q0 = qb * QBLK + wave * 16 * QI;
    const int off = p.Tk - p.Tq;  // causal: key j visible to query i iff j <= i + off
    const float sl2 = p.scale * LOG2E;
    const float xs = BIAS ? 1.f : sl2;  // units of the running max m: log2-scaled with bias, raw without

    const bf16* qbase = p.q + b * p.q_sb + h * p.q_sh;
    const u32x4 krs = make_rsrc_sgpr(p.k + b * p.k_sb + h * p.k_sh);
    const u32x4 vrs = make_rsrc_sgpr(p.v + b * p.v_sb + h * p.v_sh);

    int kv_end = p.Tk;
    if (CAUSAL) kv_end = min(p.Tk, qb * QBLK + QBLK + off);
    const int nkv = kv_end > 0 ? (kv_end + 63) / 64 : 0;
#define Kt(i) (smem + (i) * 2 * TB)
#define Vt(i) (smem + TB + (i) * 2 * TB)
    if (nkv > 0) {  // first tile in flight while Q is loaded
        stage64_async<D>(krs, p.k_st, 0, p.Tk, Kt(0), wave, lane);
        stage64_async<D>(vrs, p.v_st, 0, p.Tk, Vt(0), wave, lane);
    }

    s16x8 qf[QI][NS];
#pragma unroll
    for (int qi = 0; qi < QI; ++qi)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int row = q0 + qi * 16 + c;
            qf[qi][s] = gload16(qbase + (long)row * p.q_st + s * 32 + g * 8, row < p.Tq);
        }
    // Re-define qf through an (empty) asm so the compiler's wait for these loads happens
    // here, once: otherwise it re-waits vmcnt(0) inside the loop at their first use,
    // which would also drain the in-flight K/V prefetch.
#pragma unroll
    for (int qi = 0; qi < QI; ++qi)
#pragma unroll
        for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(qf[qi][s]));
    float m[QI], l[QI];
#pragma unroll
    for (int qi = 0; qi < QI; ++qi) { m[qi] = -INFINITY; l[qi] = 0.f; }
    f32x4 oacc[QI][NJ];
#pragma unroll
    for (int qi = 0; qi < QI; ++qi)
#pragma unroll
        for (int jd = 0; jd < NJ; ++jd) oacc[qi][jd] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const float rd = DROP ? 1.f / (1.f - p.p_drop) : 1.f;
    if (p.p_drop > 0.f && p.seed_ptr) p.seed = *p.seed_ptr;
    for (int t = 0; t < nkv; ++t) {
        vm_wait_all();   // this wave's DMA of tile t landed ...
        __syncthreads(); // ... and every wave's; every wave also finished tile t-1 (its buffer is free)
        const int cur = t & 1;
        if (t + 1 < nkv) {
            stage64_async<D>(krs, p.k_st, (t + 1) * 64, p.Tk, Kt(cur ^ 1), wave, lane);
            stage64_async<D>(vrs, p.v_st, (t + 1) * 64, p.Tk, Vt(cur ^ 1), wave, lane);
        }
        const int kv0 = t * 64;
        // wave-uniform skip: this wave's queries all precede the tile
        if (CAUSAL && kv0 > q0 + 16 * QI - 1 + off) continue;
        const char* kt = Kt(cur);
        const char* vt = Vt(cur);
        f32x4 sacc[QI][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s16x8 a[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) a[s] = rowfrag<D>(kt, j * 16 + c, s, lane);
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) {
                f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < NS; ++s) z = MFMA(a[s], qf[qi][s], z, 0, 0, 0);
                sacc[qi][j] = z;
            }
        }
        if constexpr (BIAS) {  // x = s·scale·log2e + bias·log2e
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) {
                const int qg = q0 + qi * 16 + c;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kvb = kv0 + j * 16 + 4 * g;
                    float bb[4] = {0.f, 0.f, 0.f, 0.f};
                    if (qg < p.Tq) {
                        const float* bp = p.bias + ((long)(p.bias_b > 1 ? b : 0) * p.Tq + qg) * p.Tk + kvb;
                        if (kvb + 3 < p.Tk && (p.Tk & 3) == 0) {
                            float4 t4 = *reinterpret_cast<const float4*>(bp);
                            bb[0] = t4.x; bb[1] = t4.y; bb[2] = t4.z; bb[3] = t4.w;
                        } else {
                            for (int r = 0; r < 4; ++r) bb[r] = (kvb + r < p.Tk) ? bp[r] : 0.f;
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) sacc[qi][j][r] = sacc[qi][j][r] * sl2 + bb[r] * LOG2E;
                }
            }
        }
        // masking only on diagonal / ragged tiles: a real (wave-uniform) branch — the
        // empty asm keeps hipcc from if-converting it into per-element selects on
        // every tile
        if ((kv0 + 64 > p.Tk) || (CAUSAL && kv0 + 63 > q0 + off)) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) {
                const int qg = q0 + qi * 16 + c;
                const int lim = CAUSAL ? min(qg + off, p.Tk - 1) : p.Tk - 1;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kv0 + j * 16 + 4 * g + r > lim) sacc[qi][j][r] = -INFINITY;
            }
        }
#pragma unroll
        for (int qi = 0; qi < QI; ++qi) {
            const int qg = q0 + qi * 16 + c;
            float tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, sacc[qi][j][r]);
            tmax = max4groups(tmax);
            const float mn = fmaxf(m[qi], tmax);
            const float ms = (mn == -INFINITY) ? 0.f : mn;  // fully-masked rows stay at p = 0
            const float alpha = (m[qi] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m[qi] - ms) * xs);
            const float nms = -ms * xs;
            m[qi] = mn;
            float ls = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float pv = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[qi][j][r], xs, nms));
                    ls += pv;
                    if constexpr (DROP) {
                        const int kvj = kv0 + j * 16 + 4 * g + r;
                        pv = (hash_uniform(p.seed, drop_idx(p, b, h, qg, kvj)) >= p.p_drop) ? pv * rd : 0.f;
                    }
                    sacc[qi][j][r] = pv;
                }
            l[qi] = l[qi] * alpha + ls;
#pragma unroll
            for (int jd = 0; jd < NJ; ++jd) oacc[qi][jd] *= alpha;
        }
        // O^T[d][q] += V^T[d][kv] * P^T[kv][q]
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            s16x8 pb[QI];
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) pb[qi] = pack_p(sacc[qi][2 * s], sacc[qi][2 * s + 1]);
#pragma unroll
            for (int jd = 0; jd < NJ; ++jd) {
                s16x8 a = colfrag<D>(vt, 32 * s, 16 * jd, lane);
#pragma unroll
                for (int qi = 0; qi < QI; ++qi) oacc[qi][jd] = MFMA(a, pb[qi], oacc[qi][jd], 0, 0, 0);
            }
        }
    }
#undef Kt
#undef Vt
    // epilogue
    bf16* obase = p.o + b * p.o_sb + h * p.o_sh;
#pragma unroll
    for (int qi = 0; qi < QI; ++qi) {
        const float lt = sum4groups(l[qi]);
        const int qg = q0 + qi * 16 + c;
        const float inv = lt > 0.f ? 1.f / lt : 0.f;
        if (qg < p.Tq) {
#pragma unroll
            for (int jd = 0; jd < NJ; ++jd) {
                bf16x4 o4 = {(bf16)(oacc[qi][jd][0] * inv), (bf16)(oacc[qi][jd][1] * inv),
                             (bf16)(oacc[qi][jd][2] * inv), (bf16)(oacc[qi][jd][3] * inv)};
                *reinterpret_cast<bf16x4*>(obase + (long)qg * p.o_st + jd * 16 + 4 * g) = o4;
            }
            if (g == 0)
                p.lse[((long)b * p.H + h) * p.Tq + qg] = (lt > 0.f) ? (m[qi] * xs + log2f(lt)) : INFINITY;  // base 2
        }
    }
}

// ------------------------- forward v2 (no bias / dropout) -------------------------
// D = 64, non-causal, 128 queries per workgroup (two 16-query fragments per wave), occupancy 3.
// Same data layout and fragment algebra as attn_fwd64_k; the loop is restructured:
//   * two loops — the key tiles that lie wholly below Tk (no mask) and the ragged last tile
//     (masked).  A single loop with a runtime mask branch made hipcc carry the accumulators
//     through a phi and copy 34 VGPRs per tile.
//   * the 16 transposed V reads of a tile are issued right after its QKᵀ MFMAs, so they
//     land under the softmax VALU work instead of being waited for between PV MFMAs;
//   * QKᵀ issues the k-step-0 MFMAs of all 8 output tiles before the k-step-1 ones (no
//     back-to-back dependent MFMAs).
//   * the O / l rescale by alpha = exp2(m_old - m_new) runs only when some row of the wave raised
//     its running max this tile (a wave-uniform ballot; after the first tiles the max rarely moves);
//   * the row sums of P come from the matrix cores — P·1 as two extra MFMAs per query fragment
//     against an all-ones A operand — instead of 32 v_add_f32 per tile.
// The last two trade VALU issue slots, which bound this kernel at head_dim 64, for idle MFMA /
// scalar slots; l then sums the bf16-rounded P that also feeds P·V.
// (The causal case runs attn_fwd32_k, attention_mfma32.hip.)
__global__ void __launch_bounds__(256, 3) attn_fwd64v2_k(AttnArgs p) {
    constexpr int QI = 2, QW = 16 * QI, QBLK = 64 * QI;  // query fragments per wave; queries per wave / per block
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const FragOff fo = make_fragoff(lane);
    int bh, qb;
    blk_map(p, (p.Tq + QBLK - 1) / QBLK, false, bh, qb);
    const int b = bh / p.H, h = bh % p.H;
    const int q0 = qb * QBLK + wave * QW;
    const float sl2 = p.scale * LOG2E;

    const bf16* qbase = p.q + b * p.q_sb + h * p.q_sh;
    const u32x4 krs = make_rsrc_sgpr(p.k + b * p.k_sb + h * p.k_sh);
    const u32x4 vrs = make_rsrc_sgpr(p.v + b * p.v_sb + h * p.v_sh);

    const int nkv = p.Tk > 0 ? (p.Tk + 63) / 64 : 0;
    const int nfull = min(p.Tk / 64, nkv);  // tiles [0, nfull) are Tk-complete
#define Kt(i) (smem + (i) * 16384)
#define Vt(i) (smem + 8192 + (i) * 16384)
    if (nkv > 0) {
        stage64_async(krs, p.k_st, 0, p.Tk, Kt(0), wave, lane);
        stage64_async(vrs, p.v_st, 0, p.Tk, Vt(0), wave, lane);
    }
    s16x8 qf[QI][2];
#pragma unroll
    for (int qi = 0; qi < QI; ++qi)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = q0 + qi * 16 + c;
            qf[qi][s] = gload16(qbase + (long)row * p.q_st + s * 32 + g * 8, row < p.Tq);
        }
#pragma unroll
    for (int qi = 0; qi < QI; ++qi) asm volatile("" : "+v"(qf[qi][0]), "+v"(qf[qi][1]));
    float m[QI], l[QI];
#pragma unroll
    for (int qi = 0; qi < QI; ++qi) { m[qi] = -INFINITY; l[qi] = 0.f; }
    f32x4 oacc[QI][4];
#pragma unroll
    for (int qi = 0; qi < QI; ++qi)
#pragma unroll
        for (int jd = 0; jd < 4; ++jd) oacc[qi][jd] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const short one = 0x3F80;  // bf16 1.0
    const s16x8 ones = {one, one, one, one, one, one, one, one};

    auto tile = [&](const int t, auto masked_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
        const int cur = t & 1;
        const char* kt = Kt(cur);
        const char* vt = Vt(cur);
        const int kv0 = t * 64;
        f32x4 sacc[QI][4];
        s16x8 ka[4][2];
        bool moved = false;
        float alph[QI];
        // masked tiles: a (16-query fragment qi, 16-key block j) of this wave with no visible pair —
        // past Tq / Tk (the ragged tail of a sequence) — skips its QKᵀ and P·V MFMAs (wave-uniform;
        // its scores are −inf, so P = 0 there)
        auto live = [&](int qi, int j) -> bool {
            if constexpr (!MASKED) return true;
            const int qa = q0 + qi * 16, k0 = kv0 + j * 16;
            return !(qa >= p.Tq || k0 >= p.Tk);
        };
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ka[j][0] = rowfragx(kt, j, 0, fo);
            ka[j][1] = rowfragx(kt, j, 1, fo);
        }
        if constexpr (MASKED) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int qi = 0; qi < QI; ++qi) {
                    if (live(qi, j)) {
                        sacc[qi][j] = MFMA(ka[j][0], qf[qi][0], ((f32x4){0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
                        sacc[qi][j] = MFMA(ka[j][1], qf[qi][1], sacc[qi][j], 0, 0, 0);
                    } else {
                        sacc[qi][j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    }
                }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int qi = 0; qi < QI; ++qi) sacc[qi][j] = MFMA(ka[j][0], qf[qi][0], ((f32x4){0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int qi = 0; qi < QI; ++qi) sacc[qi][j] = MFMA(ka[j][1], qf[qi][1], sacc[qi][j], 0, 0, 0);
        }
        // V^T fragments for the PV product, in flight during the softmax
        s16x8 va[2][4];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int jd = 0; jd < 4; ++jd) va[s][jd] = colfragx(vt, s, jd, fo);
        if constexpr (MASKED) {
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kv0 + j * 16 + 4 * g + r > p.Tk - 1) sacc[qi][j][r] = -INFINITY;
            }
        }
#pragma unroll
        for (int qi = 0; qi < QI; ++qi) {
            float tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, sacc[qi][j][r]);
            tmax = max4groups(tmax);
            const float mn = fmaxf(m[qi], tmax);
            float alpha, nms;
            if constexpr (MASKED) {
                const float ms = (mn == -INFINITY) ? 0.f : mn;  // fully-masked rows stay at p = 0
                alpha = (m[qi] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f((m[qi] - ms) * sl2);
                nms = -ms * sl2;
            } else {  // an unmasked tile has a finite max in every row
                alpha = __builtin_amdgcn_exp2f((m[qi] - mn) * sl2);  // exp2(-inf) = 0 on the first tile
                nms = -mn * sl2;
            }
            moved |= (mn != m[qi]);
            alph[qi] = alpha;
            m[qi] = mn;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    sacc[qi][j][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[qi][j][r], sl2, nms));
        }
        if (__builtin_amdgcn_ballot_w64(moved)) {  // wave-uniform
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) {
                l[qi] *= alph[qi];
#pragma unroll
                for (int jd = 0; jd < 4; ++jd) oacc[qi][jd] *= alph[qi];
            }
        }
        f32x4 lsum[QI];
#pragma unroll
        for (int qi = 0; qi < QI; ++qi) lsum[qi] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            s16x8 pb[QI];
#pragma unroll
            for (int qi = 0; qi < QI; ++qi) pb[qi] = pack_p(sacc[qi][2 * s], sacc[qi][2 * s + 1]);
            if constexpr (MASKED) {  // skip (qi, k-step) pairs whose 32 keys are all dead for qi
#pragma unroll
                for (int qi = 0; qi < QI; ++qi) {
                    if (!(live(qi, 2 * s) || live(qi, 2 * s + 1))) continue;
#pragma unroll
                    for (int jd = 0; jd < 4; ++jd) oacc[qi][jd] = MFMA(va[s][jd], pb[qi], oacc[qi][jd], 0, 0, 0);
                    lsum[qi] = MFMA(ones, pb[qi], lsum[qi], 0, 0, 0);
                }
            } else {
#pragma unroll
                for (int jd = 0; jd < 4; ++jd)
#pragma unroll
                    for (int qi = 0; qi < QI; ++qi) oacc[qi][jd] = MFMA(va[s][jd], pb[qi], oacc[qi][jd], 0, 0, 0);
#pragma unroll
                for (int qi = 0; qi < QI; ++qi) lsum[qi] = MFMA(ones, pb[qi], lsum[qi], 0, 0, 0);
            }
        }
#pragma unroll
        for (int qi = 0; qi < QI; ++qi) l[qi] += lsum[qi][0];  // every row of P·1 holds the sum
    };
    auto sync_prefetch = [&](int t) {
        vm_wait_all();   // this wave's DMA of tile t landed ...
        __syncthreads(); // ... and every wave's; tile t-1's buffer is free
        if (t + 1 < nkv) {
            stage64_async(krs, p.k_st, (t + 1) * 64, p.Tk, Kt((t & 1) ^ 1), wave, lane);
            stage64_async(vrs, p.v_st, (t + 1) * 64, p.Tk, Vt((t & 1) ^ 1), wave, lane);
        }
    };
    // (not unrolled by buffer like the backward kernels: at occupancy 3 the unrolled loop spills)
    // A wave whose queries all lie past Tq (the padded rows of a T = 197 sequence's last block) skips
    // every tile's work; it still joins every tile's barrier and DMA issue.
    const int nf = q0 < p.Tq ? nfull : 0;  // wave-uniform trip count
    int t = 0;
    for (; t < nf; ++t) {
        sync_prefetch(t);
        tile(t, std::false_type{});
    }
    for (; t < nkv; ++t) {
        sync_prefetch(t);
        if (q0 >= p.Tq) continue;  // wave-uniform: no live query in this wave
        tile(t, std::true_type{});
    }
#undef Kt
#undef Vt
    bf16* obase = p.o + b * p.o_sb + h * p.o_sh;
#pragma unroll
    for (int qi = 0; qi < QI; ++qi) {
        const float lt = l[qi];  // P·1 already summed over all 64 keys
        const int qg = q0 + qi * 16 + c;
        const float inv = lt > 0.f ? 1.f / lt : 0.f;
        if (qg < p.Tq) {
#pragma unroll
            for (int jd = 0; jd < 4; ++jd) {
                bf16x4 o4 = {(bf16)(oacc[qi][jd][0] * inv), (bf16)(oacc[qi][jd][1] * inv),
                             (bf16)(oacc[qi][jd][2] * inv), (bf16)(oacc[qi][jd][3] * inv)};
                *reinterpret_cast<bf16x4*>(obase + (long)qg * p.o_st + jd * 16 + 4 * g) = o4;
            }
            if (g == 0)
                p.lse[((long)b * p.H + h) * p.Tq + qg] = (lt > 0.f) ? (m[qi] * sl2 + log2f(lt)) : INFINITY;  // base 2
        }
    }
}

// the single-loop kernel at head size D (OCC / QI: see the kernel); PLAIN: with the no-bias, no-dropout forms
template <int D, int OCC, int QI, bool PLAIN>
int launch_fwd64(const AttnArgs& a, unsigned wgs, hipStream_t st) {
    auto kern = [](auto c, auto b, auto d) {
        return (const void*)attn_fwd64_k<decltype(c)::value, decltype(b)::value, decltype(d)::value, D, OCC, QI>;
    };
    return attn_launch3<PLAIN>(kern, a, wgs, 4 * kTB<D>, st);
}

}  // namespace

int attn_launch_fwd16(const AttnArgs& a, AttnPath path, unsigned wgs, hipStream_t st) {
    switch (path) {
    case AttnPath::Mfma:
        return a.D == 32 ? launch_fwd64<32, 3, 2, true>(a, wgs, st) : launch_fwd64<128, 2, 1, true>(a, wgs, st);
    case AttnPath::Plain:
        if (a.D != 64 || a.causal || a.bias || a.p_drop > 0.f) return ATTN_ERR_PATH;
        return attn_launch((const void*)attn_fwd64v2_k, dim3(wgs), 256, 32768, a, st);
    case AttnPath::BiasDrop: return launch_fwd64<64, 3, 2, false>(a, wgs, st);
    default: return ATTN_ERR_PATH;
    }
}

}  // namespace rn_attn
