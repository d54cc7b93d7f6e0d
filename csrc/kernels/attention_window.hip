// Multi-query window attention over a KV cache, head size 64: T (1..16) new tokens per batch row, row
// b's window starting at its own cache row pos[b] (speculative decoding's verify step; the same
// primitive serves any "T new queries per row, each row at its own position").  One launch does the
// append and the attention:
//   * window rows i with pos + i < L are copied, K and V, from the packed projection output
//     qkv (B, T, 3, H, 64) into kv[b, pos + i] (B, L, 2, H, 64), bit for bit; rows at or past L are
//     skipped and no other byte of the cache changes;
//   * query i attends cache rows 0 .. pos-1 and window rows 0 .. i (bottom-right-aligned causal).
// pos: B device integers (int32 / int64), clamped to [0, L] here, so no device value can index outside
// the buffer.  Cache rows at or past pos are never loaded: the window's keys / values are read from
// qkv, so stale or unwritten cache rows may hold anything (NaN bit patterns included) and there is no
// write-then-read ordering between the append and the attention.  Work and bytes follow pos[b], not L.
//
// Shape: one workgroup of 4 waves per (b, h).  The keys are one logical sequence of pos + T rows (a
// row < pos comes from the cache, the others from qkv), walked in tiles of 32; wave w takes tiles
// w, w + 4, ...  The T queries padded to 16 are the MFMA's column dimension (lane & 15) and the keys
// land in the accumulator registers, as in attention_fwd.hip: Sᵀ = K·Qᵀ is two 16-key tiles of
// v_mfma_f32_16x16x32_bf16 (accumulator: col = lane & 15, row = 4 (lane >> 4) + reg), so the online
// softmax is per lane plus two cross-group shuffles for the max, and the 8 probabilities a lane holds
// are already an operand of Oᵀ += Vᵀ·Pᵀ (operand: k = 8 (lane >> 4) + j).  The two maps differ by a
// fixed permutation of the step's 32 keys — operand slot 8 g + j is key 4 g + j (j < 4) or
// 16 + 4 g + (j - 4) — and the value tile is written to LDS transposed in that slot order, so a Vᵀ
// fragment is one 16-byte LDS read.  Every cached K / V row is loaded from memory once per (b, h),
// whatever T is.  Each wave keeps its own running max, sum and 16 × 64 output; the waves are merged
// through LDS in wave order: no atomics, two runs agree bit for bit.
#include "common.h"
#include "rn_api.h"

namespace {

constexpr int WIN_T = 256, WIN_W = 4;  // threads, waves
constexpr int WIN_VLD = 40;            // Vᵀ tile row length in bf16: 32 key slots + pad (80 B: 16-byte aligned rows)

#define WIN_MFMA __builtin_amdgcn_mfma_f32_16x16x32_bf16

RN_DEV s16x8 win_load16(const bf16* p, bool ok) {
    if (!ok) return (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
    return *reinterpret_cast<const s16x8*>(p);
}

// element strides: qkv (batch, token, q|k|v, head), cache (batch, row, k|v, head), o (batch, token, head)
struct WinStrides {
    long q_sb, q_st, q_s3, q_sh, c_sb, c_st, c_s2, c_sh, o_sb, o_st, o_sh;
};

__global__ void __launch_bounds__(WIN_T) attn_window64_k(const bf16* __restrict__ qkv, bf16* kv, const void* __restrict__ pos_p,
                                                         int pos64, bf16* __restrict__ o, int H, int T, int L,
                                                         WinStrides s, float scale) {
    __shared__ __attribute__((aligned(16))) short vt[WIN_W][64 * WIN_VLD];  // per wave: Vᵀ [d][key slot]
    __shared__ float o_s[WIN_W][64][16];                                    // per wave: Oᵀ [d][query]
    __shared__ float m_s[WIN_W][16], l_s[WIN_W][16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 4, c = lane & 15;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const long pv = pos64 ? static_cast<const int64_t*>(pos_p)[b] : (long)static_cast<const int*>(pos_p)[b];
    const int pos = (int)(pv < 0 ? 0 : (pv > L ? (long)L : pv));
    const int nk = pos + T;  // logical keys: cache rows 0 .. pos-1, then the window
    const bf16* qb = qkv + b * s.q_sb + h * s.q_sh;
    bf16* cb = kv + b * s.c_sb + h * s.c_sh;

    // the append: thread (window row, K|V, 16-byte chunk); only rows >= pos are written and only rows < pos
    // are read below (by this and every other workgroup of the batch row), so no ordering is needed
    {
        const int i = t >> 4, which = (t >> 3) & 1, ch = t & 7;
        if (i < T && pos + i < L)
            *reinterpret_cast<s16x8*>(cb + (long)(pos + i) * s.c_st + which * s.c_s2 + ch * 8) =
                *reinterpret_cast<const s16x8*>(qb + (long)i * s.q_st + (1 + which) * s.q_s3 + ch * 8);
    }

    // row kk of the logical key (which = 0) / value (which = 1) sequence; the caller checks kk < nk
    auto row = [&](int kk, int which) -> const bf16* {
        return kk < pos ? cb + (long)kk * s.c_st + which * s.c_s2
                        : qb + (long)(kk - pos) * s.q_st + (1 + which) * s.q_s3;
    };

    // Qᵀ operand: lane (query c, group g) holds q[c][32 half + 8 g .. + 7]; padded queries are zero
    s16x8 qf[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) qf[hf] = win_load16(qb + (long)c * s.q_st + hf * 32 + g * 8, c < T);

    const float sl2 = scale * 1.4426950408889634f;
    const int ntiles = (nk + 31) >> 5, iters = (ntiles + WIN_W - 1) / WIN_W;  // the same for every wave (barriers below)
    float m = -INFINITY, l = 0.f;  // log2 units; l: this lane's part of the row sum (reduced at the end)
    f32x4 oacc[4];
#pragma unroll
    for (int jd = 0; jd < 4; ++jd) oacc[jd] = (f32x4){0.f, 0.f, 0.f, 0.f};
    short* vw = vt[wave];

    for (int it = 0; it < iters; ++it) {
        const int base = (it * WIN_W + wave) * 32;  // at or past nk: a wave without a tile this round does masked work
        // K operand: lane (key c of the 16-key tile, group g) holds k[key][32 half + 8 g .. + 7]
        s16x8 ka[2][2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int kk = base + 16 * tl + c;
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) ka[tl][hf] = win_load16(row(kk, 0) + hf * 32 + g * 8, kk < nk);
        }
        // V: lane (key pair u * 8 + lane / 8, 8-column chunk lane % 8): two adjacent keys, one 32-bit LDS word each
        s16x8 va[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                const int kk = base + 2 * (u * 8 + (lane >> 3)) + e2;
                va[u][e2] = win_load16(row(kk, 1) + (lane & 7) * 8, kk < nk);
            }
        f32x4 sc[2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            sc[tl] = WIN_MFMA(ka[tl][0], qf[0], ((f32x4){0.f, 0.f, 0.f, 0.f}), 0, 0, 0);
            sc[tl] = WIN_MFMA(ka[tl][1], qf[1], sc[tl], 0, 0, 0);
        }
        // accumulator (tl, r) of this lane: key base + 16 tl + 4 g + r, query c
        bool ok[2][4];
        float tm = -INFINITY;
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kk = base + 16 * tl + 4 * g + r;
                ok[tl][r] = kk < nk && kk <= pos + c;
                sc[tl][r] = ok[tl][r] ? sc[tl][r] * sl2 : -INFINITY;
                tm = fmaxf(tm, sc[tl][r]);
            }
        tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm);
        const float alpha = (m == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        s16x8 pb;  // Pᵀ operand: slot j = accumulator (j / 4, j % 4)
        float ps = 0.f;
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bf16 p = (bf16)(ok[tl][r] ? __builtin_amdgcn_exp2f(sc[tl][r] - mn) : 0.f);
                ps += (float)p;  // the sum of what P·V multiplies
                pb[4 * tl + r] = __builtin_bit_cast(short, p);
            }
        l = l * alpha + ps;
#pragma unroll
        for (int jd = 0; jd < 4; ++jd)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[jd][r] *= alpha;
        __syncthreads();  // the previous round's fragment reads are done
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int ko = 2 * (u * 8 + (lane >> 3));  // even key offset in the tile; ko + 1 is the next slot
            const int slot = 8 * ((ko & 15) >> 2) + 4 * (ko >> 4) + (ko & 3);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *reinterpret_cast<uint32_t*>(vw + ((lane & 7) * 8 + e) * WIN_VLD + slot) =
                    (uint32_t)(uint16_t)va[u][0][e] | ((uint32_t)(uint16_t)va[u][1][e] << 16);
        }
        __syncthreads();
#pragma unroll
        for (int jd = 0; jd < 4; ++jd) {
            const s16x8 a = *reinterpret_cast<const s16x8*>(vw + (jd * 16 + c) * WIN_VLD + 8 * g);
            oacc[jd] = WIN_MFMA(a, pb, oacc[jd], 0, 0, 0);
        }
    }

    // merge the waves in wave order: accumulator (jd, r) is Oᵀ[16 jd + 4 g + r][query c]
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (g == 0) {
        m_s[wave][c] = m;
        l_s[wave][c] = l;
    }
#pragma unroll
    for (int jd = 0; jd < 4; ++jd)
#pragma unroll
        for (int r = 0; r < 4; ++r) o_s[wave][jd * 16 + 4 * g + r][c] = oacc[jd][r];
    __syncthreads();
    const int q = t & 15, d0 = (t >> 4) * 4;
    float mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < WIN_W; ++w) mx = fmaxf(mx, m_s[w][q]);
    float lt = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < WIN_W; ++w) {
        const float f = (m_s[w][q] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_s[w][q] - mx);
        lt += f * l_s[w][q];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += f * o_s[w][d0 + r][q];
    }
    if (q < T) {
        const float inv = lt > 0.f ? 1.f / lt : 0.f;
        bf16x4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = (bf16)(acc[r] * inv);
        *reinterpret_cast<bf16x4*>(o + b * s.o_sb + (long)q * s.o_st + h * s.o_sh + d0) = ov;
    }
}

}  // namespace

extern "C" int rn_attn_window(const void* qkv, void* kv, const void* pos, int pos64, void* o, int B, int T, int H,
                              int L, int D, const long* qs, const long* cs, float scale, hipStream_t st) {
    if (D != 64 || T < 1 || T > 16 || L < 1 || L > 1024 || B < 1 || H < 1) return -1;
    for (int i = 0; i < 4; ++i)
        if (qs[i] % 8 != 0 || cs[i] % 8 != 0) return -1;  // 16-byte row loads and stores
    const WinStrides s{qs[0], qs[1], qs[2], qs[3], cs[0], cs[1], cs[2], cs[3], (long)T * H * 64, (long)H * 64, 64};
    attn_window64_k<<<B * H, WIN_T, 0, st>>>((const bf16*)qkv, (bf16*)kv, pos, pos64, (bf16*)o, H, T, L, s, scale);
    return 0;
}
