// One-token attention for n samples per prompt over one shared prompt cache, head size 64, with the append
// folded in.  Batch row b = g n + s is sample s of prompt (group) g:
//   * prefix (G, P, 2, H, 64): the prompts' keys / values, read only; group g holds plen[g] rows;
//   * kv (B, L, 2, H, 64): each row's own tail — the keys / values of the tokens it has generated;
//   * the new K and V vectors of qkv (B, 1, 3, H, 64) are copied, bit for bit, to kv[b, pos[b]] if pos[b] < L
//     (otherwise nothing is written), and the query attends prefix rows < plen[g], tail rows < pos[b] and its
//     own new row, which is taken from qkv and never re-read from memory: the append and the attention need
//     no ordering (the rule of attention_window.hip).
// plen (G,) and pos (B,) are device integers (int32 / int64) clamped here to [0, P] and [0, L], so no device
// value can index outside a buffer.  Prefix rows at or past plen[g] and tail rows at or past pos[b] are never
// loaded: they may hold anything (NaN bit patterns included), and work and bytes follow plen and pos, not P
// and L.  No atomics, a fixed reduction order: two runs agree bit for bit.
//
// Two launches; the launch boundary is the only ordering between them.
//   1. prefix_partials64_k, one workgroup of 4 waves per (g, h, key split).  The samples of the group are the
//      MFMA's column dimension in blocks of 16, exactly attn_window64_k's arrangement (Sᵀ = K·Qᵀ as two 16-key
//      tiles of v_mfma_f32_16x16x32_bf16, the probabilities feeding Oᵀ += Vᵀ·Pᵀ from the accumulator registers,
//      the value tile transposed through LDS in operand-slot order); for n > 16 the wave walks its NQB query
//      blocks over the key / value fragments it has already loaded, so a prefix row is read from memory once
//      per (g, h, split), not once per sample.  The prefix rows are cut into `splits` equal ranges of `chunk`
//      rows — both functions of the host-known shapes only (prefix_plan), so a captured graph is fixed — and a
//      split whose range starts at or past plen[g] writes an empty partial (m = -inf, l = 0) and returns.
//      Wave w takes the split's 32-key tiles w, w + 4, ...; the waves are merged through LDS in wave order
//      and the split writes fp32 (m, l, O[64]) per (b, h), unnormalised, m in log2 units.
//   2. prefix_tail_merge64_k, one workgroup per (b, h): the append; the row's own tail in the lens form of
//      attn_decode64_k (one key per thread, P·V by 32 key groups summed in order); then the merge — the
//      split partials in split order, the tail, the new row — and the normalisation.
// Workspace (fp32): O[splits][B H][64], then (m, l)[splits][B H][2].
#include "common.h"
#include "rn_api.h"

namespace {

constexpr int PFX_T = 256, PFX_W = 4;  // threads, waves
constexpr int PFX_VLD = 40;            // Vᵀ tile row length in bf16: 32 key slots + pad (80 B: 16-byte aligned rows)
constexpr int PFX_KPT = 4;             // tail keys per thread: L <= 4 · 256
constexpr int PFX_MAX_P = 1024, PFX_MAX_L = PFX_T * PFX_KPT, PFX_MAX_N = 64;
constexpr float LOG2E = 1.4426950408889634f;

#define PFX_MFMA __builtin_amdgcn_mfma_f32_16x16x32_bf16

RN_DEV s16x8 pfx_load16(const bf16* p, bool ok) {
    if (!ok) return (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
    return *reinterpret_cast<const s16x8*>(p);
}

RN_DEV int pfx_clamped(const void* p, int is64, long i, int hi) {
    const long v = is64 ? static_cast<const int64_t*>(p)[i] : (long)static_cast<const int*>(p)[i];
    return (int)(v < 0 ? 0 : (v > hi ? (long)hi : v));
}

// element strides: qkv (batch, q|k|v, head), prefix (group, row, k|v, head), tail (batch, row, k|v, head)
struct PfxStrides {
    long q_sb, q_s3, q_sh, p_sg, p_st, p_s2, p_sh, c_sb, c_st, c_s2, c_sh;
};

// the split plan: a function of the host-known shapes only.  Enough workgroups to cover the CUs twice where
// G · H alone does not, a split no shorter than one tile per wave (128 rows), the chunk a multiple of the tile.
struct PfxPlan {
    int splits, chunk;
};
PfxPlan prefix_plan(int G, int H, int /*n*/, int P) {
    const int most = (P + 127) / 128, want = (512 + G * H - 1) / (G * H);
    int S = want < most ? want : most;
    if (S < 1) S = 1;
    const int chunk = ((P + S - 1) / S + 31) / 32 * 32;
    return {(P + chunk - 1) / chunk, chunk};
}

template <int NQB>
__global__ void __launch_bounds__(PFX_T) prefix_partials64_k(const bf16* __restrict__ qkv, const bf16* __restrict__ pkv,
                                                             const void* __restrict__ plen_p, int plen64,
                                                             float* __restrict__ ws, int H, int n, int P, int S,
                                                             int chunk, long BH, PfxStrides s, float scale) {
    __shared__ __attribute__((aligned(16))) short vt[PFX_W][64 * PFX_VLD];  // per wave: Vᵀ [d][key slot]
    __shared__ float o_s[PFX_W][64][16];                                    // per wave: Oᵀ [d][query]
    __shared__ float m_s[PFX_W][16], l_s[PFX_W][16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, c = lane & 15;
    const int sp = blockIdx.x % S, gh = blockIdx.x / S, grp = gh / H, h = gh % H;
    const int plen = pfx_clamped(plen_p, plen64, grp, P);
    const int k0 = sp * chunk, k1 = min(k0 + chunk, plen);  // this split's prefix rows
    float* wo = ws + (long)sp * BH * 64;
    float* wml = ws + (long)S * BH * 64 + (long)sp * BH * 2;
    const long b0 = (long)grp * n;  // the group's first batch row
    if (k0 >= plen) {                // nothing to read (uniform over the workgroup: before any barrier)
        if (t < n) {
            wml[((b0 + t) * H + h) * 2] = -INFINITY;
            wml[((b0 + t) * H + h) * 2 + 1] = 0.f;
        }
        return;
    }
    const bf16* pb_ = pkv + grp * s.p_sg + h * s.p_sh;
    const bf16* qb = qkv + b0 * s.q_sb + h * s.q_sh;

    // Qᵀ operands: lane (query c of block j, group g) holds q[16 j + c][32 half + 8 g .. + 7]; padded queries are zero
    s16x8 qf[NQB][2];
#pragma unroll
    for (int j = 0; j < NQB; ++j)
#pragma unroll
        for (int hf = 0; hf < 2; ++hf)
            qf[j][hf] = pfx_load16(qb + (long)(16 * j + c) * s.q_sb + hf * 32 + g * 8, 16 * j + c < n);

    const float sl2 = scale * LOG2E;
    const int ntiles = (k1 - k0 + 31) >> 5, iters = (ntiles + PFX_W - 1) / PFX_W;  // the same for every wave (barriers below)
    float m[NQB], l[NQB];  // log2 units; l: this lane's part of the row sum (reduced at the end)
    f32x4 oacc[NQB][4];
#pragma unroll
    for (int j = 0; j < NQB; ++j) {
        m[j] = -INFINITY;
        l[j] = 0.f;
#pragma unroll
        for (int jd = 0; jd < 4; ++jd) oacc[j][jd] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    short* vw = vt[wave];

    for (int it = 0; it < iters; ++it) {
        const int base = k0 + (it * PFX_W + wave) * 32;  // at or past k1: a wave without a tile this round does masked work
        // K operand: lane (key c of the 16-key tile, group g) holds k[key][32 half + 8 g .. + 7]
        s16x8 ka[2][2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int kk = base + 16 * tl + c;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) ka[tl][hf] = pfx_load16(pb_ + (long)kk * s.p_st + hf * 32 + g * 8, kk < k1);
        }
        // V: lane (key pair u * 8 + lane / 8, 8-column chunk lane % 8): two adjacent keys, one 32-bit LDS word each
        s16x8 va[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                const int kk = base + 2 * (u * 8 + (lane >> 3)) + e2;
                va[u][e2] = pfx_load16(pb_ + (long)kk * s.p_st + s.p_s2 + (lane & 7) * 8, kk < k1);
            }
        // accumulator (tl, r) of this lane: key base + 16 tl + 4 g + r, query c of each block
        bool ok[2][4];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
            for (int r = 0; r < 4; ++r) ok[tl][r] = base + 16 * tl + 4 * g + r < k1;
        s16x8 pb[NQB];  // Pᵀ operands: slot j = accumulator (j / 4, j % 4)
#pragma unroll
        for (int j = 0; j < NQB; ++j) {
            f32x4 sc[2];
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                sc[tl] = PFX_MFMA(ka[tl][0], qf[j][0], ((f32x4){0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
                sc[tl] = PFX_MFMA(ka[tl][1], qf[j][1], sc[tl], 0, 0, 0);
            }
            float tm = -INFINITY;
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[tl][r] = ok[tl][r] ? sc[tl][r] * sl2 : -INFINITY;
                    tm = fmaxf(tm, sc[tl][r]);
                }
            tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const float mn = fmaxf(m[j], tm);  // -inf only while the wave has seen no key: every p below is then 0
            const float alpha = (m[j] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m[j] - mn);
            m[j] = mn;
            float ps = 0.f;
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bf16 p = (bf16)(ok[tl][r] ? __builtin_amdgcn_exp2f(sc[tl][r] - mn) : 0.f);
                    ps += (float)p;  // the sum of what P·V multiplies
                    pb[j][4 * tl + r] = __builtin_bit_cast(short, p);
                }
            l[j] = l[j] * alpha + ps;
#pragma unroll
            for (int jd = 0; jd < 4; ++jd)
#pragma unroll
                for (int r = 0; r < 4; ++r) oacc[j][jd][r] *= alpha;
        }
        __syncthreads();  // the previous round's fragment reads are done
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ko = 2 * (u * 8 + (lane >> 3));  // even key offset in the tile; ko + 1 is the next slot
            const int slot = 8 * ((ko & 15) >> 2) + 4 * (ko >> 4) + (ko & 3);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *reinterpret_cast<uint32_t*>(vw + ((lane & 7) * 8 + e) * PFX_VLD + slot) =
                    (uint32_t)(uint16_t)va[u][0][e] | ((uint32_t)(uint16_t)va[u][1][e] << 16);
        }
        __syncthreads();
#pragma unroll
        for (int jd = 0; jd < 4; ++jd) {
            const s16x8 a = *reinterpret_cast<const s16x8*>(vw + (jd * 16 + c) * PFX_VLD + 8 * g);
#pragma unroll
            for (int j = 0; j < NQB; ++j) oacc[j][jd] = PFX_MFMA(a, pb[j], oacc[j][jd], 0, 0, 0);
        }
    }

    // per query block: merge the waves in wave order — accumulator (jd, r) is Oᵀ[16 jd + 4 g + r][query c] — and
    // write the split's partial, unnormalised
    const int q = t & 15, d0 = (t >> 4) * 4;
#pragma unroll
    for (int j = 0; j < NQB; ++j) {
        float lj = l[j];
        lj += __shfl_xor(lj, 16, 64);
        lj += __shfl_xor(lj, 32, 64);
        if (j) __syncthreads();  // the previous block's reads of o_s / m_s / l_s are done
        if (g == 0) {
            m_s[wave][c] = m[j];
            l_s[wave][c] = lj;
        }
#pragma unroll
        for (int jd = 0; jd < 4; ++jd)
#pragma unroll
            for (int r = 0; r < 4; ++r) o_s[wave][jd * 16 + 4 * g + r][c] = oacc[j][jd][r];
        __syncthreads();
        float mx = -INFINITY;
#pragma unroll
        for (int w = 0; w < PFX_W; ++w) mx = fmaxf(mx, m_s[w][q]);
        float lt = 0.f;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < PFX_W; ++w) {
            const float f = (m_s[w][q] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_s[w][q] - mx);
            lt += f * l_s[w][q];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += f * o_s[w][d0 + r][q];
        }
        if (16 * j + q < n) {
            const long bh = (b0 + 16 * j + q) * H + h;
            *reinterpret_cast<f32x4*>(wo + bh * 64 + d0) = acc;
            if (d0 == 0) {
                wml[bh * 2] = mx;
                wml[bh * 2 + 1] = lt;
            }
        }
    }
}

__global__ void __launch_bounds__(PFX_T) prefix_tail_merge64_k(const bf16* __restrict__ qkv, bf16* kv,
                                                               const void* __restrict__ pos_p, int pos64,
                                                               const float* __restrict__ ws, bf16* __restrict__ o, int H,
                                                               int L, int S, long BH, PfxStrides s, float scale) {
    __shared__ float p_s[PFX_T * PFX_KPT];
    __shared__ float red[PFX_W];
    __shared__ float part[32][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int pos = pfx_clamped(pos_p, pos64, b, L);
    const bf16* qp = qkv + b * s.q_sb + h * s.q_sh;
    const bf16 *kn = qp + s.q_s3, *vn = qp + 2 * s.q_s3;  // the new row
    bf16* cb = kv + b * s.c_sb + h * s.c_sh;

    // the append: thread (K|V, 16-byte chunk).  Only row pos is written and only rows < pos are read below (by this
    // and every other workgroup of the batch row), so no ordering is needed
    if (t < 16 && pos < L) {
        const int which = t >> 3, ch = t & 7;
        *reinterpret_cast<s16x8*>(cb + (long)pos * s.c_st + which * s.c_s2 + ch * 8) =
            *reinterpret_cast<const s16x8*>(qp + (1 + which) * s.q_s3 + ch * 8);
    }

    const float sl2 = scale * LOG2E;
    // q (64 elements) in every thread's registers; the new row's score in every thread
    float qf[64];
#pragma unroll
    for (int c = 0; c < 8; ++c) load8(qp + c * 8, qf + c * 8);
    float sn = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float kf[8];
        load8(kn + c * 8, kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) sn = fmaf(qf[c * 8 + e], kf[e], sn);
    }
    sn *= sl2;
    // the tail: rows 0 .. pos-1 of this batch row, one key per thread
    float m = -INFINITY;
    float sc[PFX_KPT];
#pragma unroll
    for (int i = 0; i < PFX_KPT; ++i) {
        const int j = t + i * PFX_T;
        sc[i] = -INFINITY;
        if (j < pos) {
            const bf16* kr = cb + (long)j * s.c_st;
            float a = 0.f, kf[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                load8(kr + c * 8, kf);
#pragma unroll
                for (int e = 0; e < 8; ++e) a = fmaf(qf[c * 8 + e], kf[e], a);
            }
            sc[i] = a * sl2;  // log2 units
        }
        m = fmaxf(m, sc[i]);
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // -inf: no tail row
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < PFX_KPT; ++i) {
        const float pv = (sc[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(sc[i] - m);
        p_s[t + i * PFX_T] = pv;
        l += pv;
    }
    l = wave_sum(l);
    __syncthreads();  // red[] read by every thread above; p_s complete
    if (lane == 0) red[wave] = l;
    __syncthreads();
    l = red[0] + red[1] + red[2] + red[3];
    // P·V: thread (8-column chunk t % 8, key group t / 8) over keys t/8, t/8 + 32, ...; the 32 groups summed in order
    const int dc = t & 7, kgp = t >> 3;
    const bf16* vb = cb + s.c_s2 + dc * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = kgp; j < pos; j += 32) {
        float vf[8];
        load8(vb + (long)j * s.c_st, vf);
        const float pj = p_s[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, vf[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[kgp][dc * 8 + e] = acc[e];
    __syncthreads();
    if (t < 64) {
        // the merge: the split partials in split order, the tail, the new row.  An empty part (m = -inf) has
        // weight 0 and its O is not read (an empty split does not write one)
        const long bh = (long)b * H + h;
        const float* wo = ws + bh * 64 + t;
        const float* wml = ws + (long)S * BH * 64 + bh * 2;
        float mx = fmaxf(m, sn);
        for (int sp = 0; sp < S; ++sp) mx = fmaxf(mx, wml[(long)sp * BH * 2]);
        float num = 0.f, den = 0.f;
        for (int sp = 0; sp < S; ++sp) {
            const float ms = wml[(long)sp * BH * 2];
            if (ms != -INFINITY) {
                const float f = __builtin_amdgcn_exp2f(ms - mx);
                den += f * wml[(long)sp * BH * 2 + 1];
                num += f * wo[(long)sp * BH * 64];
            }
        }
        if (m != -INFINITY) {
            float tot = 0.f;
            for (int gk = 0; gk < 32; ++gk) tot += part[gk][t];
            const float f = __builtin_amdgcn_exp2f(m - mx);
            den += f * l;
            num += f * tot;
        }
        const float fn = __builtin_amdgcn_exp2f(sn - mx);  // sn <= mx and finite: the new row is always attended
        den += fn;
        num += fn * bf2f(vn[t]);
        o[bh * 64 + t] = (bf16)(num / den);
    }
}

}  // namespace

extern "C" long rn_attn_prefix_ws_floats(int G, int n, int H, int P) {
    if (G < 1 || n < 1 || H < 1 || P < 1) return 0;
    return (long)prefix_plan(G, H, n, P).splits * G * n * H * 66;
}

extern "C" int rn_attn_decode_prefix(const void* qkv, const void* prefix_kv, const void* prefix_len, int plen64, void* kv,
                                     const void* pos, int pos64, float* ws, void* o, int G, int n, int H, int P, int L,
                                     int D, const long* qs, const long* ps, const long* cs, float scale,
                                     hipStream_t st) {
    if (D != 64 || G < 1 || H < 1 || n < 1 || n > PFX_MAX_N || P < 1 || P > PFX_MAX_P || L < 1 || L > PFX_MAX_L)
        return -1;
    for (int i = 0; i < 4; ++i)
        if ((i < 3 && qs[i] % 8 != 0) || ps[i] % 8 != 0 || cs[i] % 8 != 0) return -1;  // 16-byte row loads and stores
    const PfxStrides s{qs[0], qs[1], qs[2], ps[0], ps[1], ps[2], ps[3], cs[0], cs[1], cs[2], cs[3]};
    const PfxPlan plan = prefix_plan(G, H, n, P);
    const long BH = (long)G * n * H;
    const int grid = G * H * plan.splits;
#define PFX_LAUNCH(NQB)                                                                                              \
    prefix_partials64_k<NQB><<<grid, PFX_T, 0, st>>>((const bf16*)qkv, (const bf16*)prefix_kv, prefix_len, plen64, ws, H, \
                                                     n, P, plan.splits, plan.chunk, BH, s, scale)
    switch ((n + 15) / 16) {
        case 1: PFX_LAUNCH(1); break;
        case 2: PFX_LAUNCH(2); break;
        case 3: PFX_LAUNCH(3); break;
        default: PFX_LAUNCH(4); break;
    }
#undef PFX_LAUNCH
    prefix_tail_merge64_k<<<(int)BH, PFX_T, 0, st>>>((const bf16*)qkv, (bf16*)kv, pos, pos64, ws, (bf16*)o, H, L,
                                                     plan.splits, BH, s, scale);
    return 0;
}
