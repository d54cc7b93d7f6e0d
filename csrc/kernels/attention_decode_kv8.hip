// The fp8 KV cache (decoding.KVCache(kv_dtype="fp8")), head size 64: the one-token attention with the append
// folded in, and the prefill's append.
//
// Storage per layer: kv8 (B, L, 2, H, 64) OCP e4m3fn bytes and kv_scale (B, L, 2, H) fp32, one scale per
// 64-element head row: scale = pow2_ceil(amax / 448) (common.h; 1 for an all-zero row), byte = e4m3(x · (1 / scale))
// rounded to nearest even, saturating; the value read back is decode(byte) · scale.  A scale is a power of two, so
// x · (1 / scale) is exact and every byte follows from the bf16 input alone (tests/test_kv_fp8*.py compare bitwise).
// A row carries its own scale: the append needs no state and no calibration, and 68 bytes replace 128.
//
// attn_decode_kv8_k is attention_decode.hip's kernel over such a cache: one workgroup per (b, h), one key per
// thread in the score phase (the q vector in registers, 4 × 16-byte loads of the key row, v_cvt_pk_f32_fp8), the
// key's scale folded into the score after the dot product and the value row's scale into p[j] before P·V, so no
// element is multiplied by a scale.  P·V: thread (16-column chunk t % 4, key group t / 4), one 16-byte value load
// per key, the 64 groups merged in LDS in a fixed order.  No atomics: two runs agree bit for bit.
//
// The append: pos (1 or B device integers, clamped to [0, L] here, so no device value can index outside the
// buffers) is row b's write row; a negative one counts as 0 cached rows and writes nothing.  Threads 0..7
// quantise the new K and V rows (kv8_quant16: 4 lanes a row) and, if pos < L, write their 64 bytes and scale
// to row pos.  The query attends rows 0 .. pos-1 and the new row, which enters with its quantised-then-dequantised
// value from LDS, never re-read from memory: a key has one value whenever it is read, and no write-then-read
// ordering is needed.  Rows at or past pos are never loaded, neither bytes nor scales, so they may hold anything.
// Work and bytes follow pos[b], not L.
//
// Measured (profiles/decode_kv_fp8.txt; GPT-2-small, batch 64, per layer, from a kernel trace of the captured step,
// the quantise and append included): 27.5 µs at 896 - 927 cached rows, where the bf16 kernel takes 42.2 µs in its
// lens form and 45.4 µs in the masked form the uniform bf16 step runs; 8.9 µs against 9.7 / 12.4 µs at 128 - 159.
// That is 94 MB at 3.4 TB/s against 176 MB at 4.2 TB/s: not yet bound by bytes alone.
#include "common.h"
#include "rn_api.h"

namespace {

constexpr int KV8_T = 256, KV8_KPT = 4;  // threads, keys per thread in the score phase
constexpr float KV8_MAX = 448.f;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// the 4 values of one 32-bit word of e4m3 bytes, in memory order
RN_DEV void kv8_dec4(int w, float* f) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
    f[0] = lo[0], f[1] = lo[1], f[2] = hi[0], f[3] = hi[1];
}
RN_DEV void kv8_dec16(i32x4 w, float* f) {
#pragma unroll
    for (int u = 0; u < 4; ++u) kv8_dec4(w[u], f + 4 * u);
}

// One 64-element head row quantised by 4 adjacent lanes (all four active): this lane's 16 elements at src ->
// its 16 bytes; returns the row's scale.
RN_DEV float kv8_quant16(const bf16* src, i32x4& bytes) {
    float f[16];
    load8(src, f);
    load8(src + 8, f + 8);
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) a = fmaxf(a, fabsf(f[e]));
    a = fmaxf(a, __shfl_xor(a, 1, 64));
    a = fmaxf(a, __shfl_xor(a, 2, 64));
    const float scale = a > 0.f ? pow2_ceil(a / KV8_MAX) : 1.f;
    const float inv = 1.f / scale;
#pragma unroll
    for (int e = 0; e < 16; ++e) f[e] = fminf(fmaxf(f[e] * inv, -KV8_MAX), KV8_MAX);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * u], f[4 * u + 1], w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * u + 2], f[4 * u + 3], w, true);
        bytes[u] = w;
    }
    return scale;
}

// pos[i] as a row count in [0, L]; writes: whether the position is one at all (a negative one writes nothing)
RN_DEV int kv8_pos(const void* pos, int pos64, long i, int L, bool& writes) {
    const long v = pos64 ? static_cast<const int64_t*>(pos)[i] : (long)static_cast<const int*>(pos)[i];
    writes = v >= 0;
    return (int)(v < 0 ? 0 : (v > L ? (long)L : v));
}

// qkv element strides (batch, q|k|v, head); cache byte strides (batch, row, k|v, head); kv_scale contiguous.
// pos_stride: 0 (one position for the batch) or 1.
__global__ void __launch_bounds__(KV8_T) attn_decode_kv8_k(const bf16* __restrict__ qkv, uint8_t* kv8, float* kv_scale,
                                                           const void* __restrict__ pos_p, int pos64, int pos_stride,
                                                           bf16* __restrict__ o, int H, int L, long q_sb, long q_s3,
                                                           long q_sh, long c_sb, long c_st, long c_s2, long c_sh,
                                                           float scale) {
    __shared__ float p_s[KV8_T * KV8_KPT];  // p[j] · the value row's scale
    __shared__ float red[KV8_T / 64];
    __shared__ __attribute__((aligned(16))) float part[64][64];
    __shared__ float new_f[2][64];  // the new K / V row: decode(byte)
    __shared__ float new_sc[2];     // and its scales
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // A head row is 64 bytes: heads 2g and 2g + 1 share every 128-byte line of a cache row.  Workgroups are dealt
    // round-robin over the 8 XCDs (observed, not documented; a permutation of the workgroups, so for speed only),
    // so the two of a pair are made blockIdx i and i + 8: the same XCD, one after the other, and the line's second
    // half comes from that XCD's L2.  Worth about 3 µs a layer in the step at 896 rows (1.307 -> 1.269 ms per step,
    // measured before the key loads were batched).
    int bid = blockIdx.x;
    if ((H & 1) == 0 && bid < (int)(gridDim.x & ~15u)) {
        const int x = bid & 7, k = bid >> 3;
        bid = ((((k >> 1) << 3) + x) << 1) + (k & 1);
    }
    const int b = bid / H, h = bid % H;
    bool writes;
    const int n = kv8_pos(pos_p, pos64, (long)b * pos_stride, L, writes);  // cached rows this query reads; its write row
    const bf16* qb = qkv + b * q_sb + h * q_sh;
    uint8_t* cb = kv8 + b * c_sb + h * c_sh;
    float* sb = kv_scale + (long)b * L * 2 * H + h;  // scale of (row j, K|V w): sb[(2 j + w) H]

    // the append: thread (K|V, 16-element chunk).  Only row n is written and only rows < n are read below (by
    // this and every other workgroup of the batch row)
    if (t < 8) {
        const int which = t >> 2, sub = t & 3;
        i32x4 by;
        const float sc = kv8_quant16(qb + (1 + which) * q_s3 + sub * 16, by);
        kv8_dec16(by, &new_f[which][sub * 16]);
        if (sub == 0) new_sc[which] = sc;
        if (writes && n < L) {
            *reinterpret_cast<i32x4*>(cb + (long)n * c_st + which * c_s2 + sub * 16) = by;
            if (sub == 0) sb[((long)n * 2 + which) * H] = sc;
        }
    }

    const float sl2 = scale * 1.4426950408889634f;
    // q (64 elements) in every thread's registers
    float qf[64];
#pragma unroll
    for (int c = 0; c < 8; ++c) load8(qb + c * 8, qf + c * 8);
    float m = -INFINITY;
    float sc[KV8_KPT], vs[KV8_KPT];
    // Every load of the thread's (up to) 4 keys is issued before the first is used: a row is 64 bytes, and with one
    // key's loads in flight at a time a thread has half the bytes outstanding that the bf16 kernel has.  The branch
    // is uniform over the workgroup (pass i has a key at all) and the row index is clamped to n - 1, a row below
    // pos, so no lane branches around a load and no row at or past pos is read.
    i32x4 kw[KV8_KPT][4];
    float ks[KV8_KPT];
#pragma unroll
    for (int i = 0; i < KV8_KPT; ++i) {
        sc[i] = -INFINITY;
        vs[i] = 0.f;
        if (i * KV8_T < n) {
            const long jc = min(t + i * KV8_T, n - 1);
            const uint8_t* kr = cb + jc * c_st;
#pragma unroll
            for (int c = 0; c < 4; ++c) kw[i][c] = *reinterpret_cast<const i32x4*>(kr + c * 16);
            ks[i] = sb[jc * 2 * H];
            vs[i] = sb[(jc * 2 + 1) * H];
        }
    }
#pragma unroll
    for (int i = 0; i < KV8_KPT; ++i) {
        if (i * KV8_T < n) {
            float s = 0.f, kf[16];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                kv8_dec16(kw[i][c], kf);
#pragma unroll
                for (int e = 0; e < 16; ++e) s = fmaf(qf[c * 16 + e], kf[e], s);
            }
            if (t + i * KV8_T < n) sc[i] = s * ks[i] * sl2;  // log2 units
            else vs[i] = 0.f;
        }
        m = fmaxf(m, sc[i]);
    }
    __syncthreads();  // new_f, new_sc
    // the new row's score, by every wave alike
    const float s_new = wave_sum((float)qb[lane] * new_f[0][lane]) * new_sc[0] * sl2;
    m = fmaxf(wave_max(m), s_new);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < KV8_KPT; ++i) {
        const float pv = (sc[i] == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(sc[i] - m);
        p_s[t + i * KV8_T] = pv * vs[i];
        l += pv;
    }
    l = wave_sum(l);
    __syncthreads();  // red[] read by every thread above; p_s complete
    if (lane == 0) red[wave] = l;
    __syncthreads();
    const float p_new = __builtin_amdgcn_exp2f(s_new - m);
    l = red[0] + red[1] + red[2] + red[3] + p_new;
    // P·V: thread (16-column chunk t % 4, key group t / 4) over keys t/4, t/4 + 64, ...: one 16-byte value load
    // per key, at most n / 64 independent iterations per thread; the 64 groups are summed in order, then the new row
    const int dc = t & 3, kgp = t >> 2;
    const uint8_t* vb = cb + c_s2 + dc * 16;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll 4
    for (int j = kgp; j < n; j += 64) {
        float vf[16];
        kv8_dec16(*reinterpret_cast<const i32x4*>(vb + (long)j * c_st), vf);
        const float pj = p_s[j];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = fmaf(pj, vf[e], acc[e]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
        *reinterpret_cast<f32x4*>(&part[kgp][dc * 16 + 4 * u]) =
            (f32x4){acc[4 * u], acc[4 * u + 1], acc[4 * u + 2], acc[4 * u + 3]};
    __syncthreads();
    if (t < 64) {
        float tot = 0.f;
        for (int g = 0; g < 64; ++g) tot += part[g][t];
        tot = fmaf(p_new * new_sc[1], new_f[1][t], tot);
        o[((long)b * H + h) * 64 + t] = (bf16)(tot / l);  // l >= p_new of the largest score = 1
    }
}

// the prefill's append: 4 lanes per 64-element head row (b, i, K|V, h) of kv_new, 16-byte stores of the bytes
__global__ void __launch_bounds__(256) kv8_append_k(const bf16* __restrict__ x, uint8_t* __restrict__ kv8,
                                                    float* __restrict__ kv_scale, const void* __restrict__ pos_p,
                                                    int pos64, int pos_stride, int T, int H, int L, long rows, long n_sb,
                                                    long n_st, long n_s2, long n_sh, long c_sb, long c_st, long c_s2,
                                                    long c_sh) {
    const long r = (blockIdx.x * 256L + threadIdx.x) >> 2;  // head row; its 4 lanes stay or leave together
    const int sub = threadIdx.x & 3;
    if (r >= rows) return;
    const int h = (int)(r % H), which = (int)((r / H) & 1), i = (int)((r / (2L * H)) % T);
    const long b = r / (2L * H * T);
    bool writes;
    const long row = (long)kv8_pos(pos_p, pos64, b * pos_stride, L, writes) + i;
    i32x4 by;
    const float sc = kv8_quant16(x + b * n_sb + i * n_st + which * n_s2 + h * n_sh + sub * 16, by);
    if (writes && row < L) {
        *reinterpret_cast<i32x4*>(kv8 + b * c_sb + row * c_st + which * c_s2 + h * c_sh + sub * 16) = by;
        if (sub == 0) kv_scale[((b * L + row) * 2 + which) * H + h] = sc;
    }
}

bool kv8_strides_ok(const long* xs, int nx, const long* cs) {
    for (int i = 0; i < nx; ++i)
        if (xs[i] % 8 != 0 || xs[i] < 0) return false;  // 16-byte bf16 loads
    for (int i = 0; i < 4; ++i)
        if (cs[i] % 16 != 0 || cs[i] < 0) return false;  // 16-byte loads and stores of the bytes
    return true;
}

}  // namespace

extern "C" int rn_attn_decode_kv8(const void* qkv, void* kv8, float* kv_scale, const void* pos, int pos64, int pos_n,
                                  void* o, int B, int H, int L, int D, const long* qs, const long* cs, float scale,
                                  hipStream_t st) {
    if (D != 64 || L < 1 || L > KV8_T * KV8_KPT || B < 1 || H < 1 || (pos_n != 1 && pos_n != B)) return -1;
    if ((long)B * H > (1L << 30) || !kv8_strides_ok(qs, 3, cs)) return -1;
    attn_decode_kv8_k<<<B * H, KV8_T, 0, st>>>((const bf16*)qkv, (uint8_t*)kv8, kv_scale, pos, pos64, pos_n == 1 ? 0 : 1,
                                               (bf16*)o, H, L, qs[0], qs[1], qs[2], cs[0], cs[1], cs[2], cs[3], scale);
    return 0;
}

extern "C" int rn_kv8_append(const void* kv_new, void* kv8, float* kv_scale, const void* pos, int pos64, int pos_n,
                             int B, int T, int H, int L, int D, const long* ns, const long* cs, hipStream_t st) {
    if (D != 64 || L < 1 || L > (1 << 30) || B < 1 || T < 1 || H < 1 || (pos_n != 1 && pos_n != B)) return -1;
    const long rows = (long)B * T * 2 * H;
    if (rows > (1L << 28) || !kv8_strides_ok(ns, 4, cs)) return -1;
    kv8_append_k<<<rn_cdiv(rows * 4, 256), 256, 0, st>>>((const bf16*)kv_new, (uint8_t*)kv8, kv_scale, pos, pos64,
                                                         pos_n == 1 ? 0 : 1, T, H, L, rows, ns[0], ns[1], ns[2], ns[3],
                                                         cs[0], cs[1], cs[2], cs[3]);
    return 0;
}
