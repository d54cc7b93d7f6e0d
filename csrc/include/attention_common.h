// What the attention translation units share (csrc/kernels/attention*.hip, attention_decode.hip excepted):
// the argument block, the device helpers that more than one kernel family uses, and the plain launcher
// functions through which the host code in attention.hip reaches each family's kernels.  Kernels and their
// templates stay inside the units; a helper that only one family uses stays with that family.
#pragma once

#include "common.h"

#include <type_traits>

namespace rn_attn {

constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

struct AttnArgs {
    const bf16* q; const bf16* k; const bf16* v; bf16* o; float* lse; const float* bias;
    const bf16* dout; bf16* dq; bf16* dk; bf16* dv; const float* delta;
    long q_sb, q_st, q_sh, k_sb, k_st, k_sh, v_sb, v_st, v_sh, o_sb, o_st, o_sh;
    long do_sb, do_st, do_sh, dq_sb, dq_st, dq_sh, dk_sb, dk_st, dk_sh, dv_sb, dv_st, dv_sh;
    int B, H, Tq, Tk, D;
    int causal, bias_b;
    float scale, p_drop;
    uint64_t seed;
    // optional device seed (graph-capturable dropout: drawn on the device per call, see ops/rng.py);
    // replaces `seed` when set
    const uint64_t* seed_ptr;
    // 16 unused bytes (a former scratch-pointer pair): they keep the kernel-argument offsets of the fields
    // below, and with them every backward kernel's scalar-load grouping and register allocation, where the
    // measured code has them; closing the gap re-schedules some fifty kernels and has to be timed
    uint64_t reserved_[2];
    // optional [B * ceil(T/64)][3 * H * 64] fp32: per-64-row-block column sums of dQ | dK | dV
    // (the packed-QKV projection's bias gradient, reduced later) — fast path, self-attention
    float* bsum;
    // lse units: the D = 64 forward kernels store log2(Σ exp) in base-2 units (the backward then
    // needs one FMA per score, exp2(s·scale·log2e − lse2)); the generic forward stores natural log.
    int lse_log2;
    // optional (D = 64 fast path): dQ | dK | dV also — or, q8_only, only — as OCP e5m2 at q8 (same element
    // offsets as dq / dk / dv: the packed dQKV's byte image) with the fp8 consumer's delayed scale q8st[0]
    // (rolled before the launch); amax(|dQKV|) recorded into q8st[1].  The c_attn projection's fp8 data /
    // weight gradients then need no quantisation pass over dQKV.
    uint8_t* q8;   // dQ's e5m2 base (dK / dV: q8k / q8v, the same element offsets as dk / dv)
    uint8_t* q8k;
    uint8_t* q8v;
    float* q8st;
    int q8_only;
    // per-wave amax partials (no same-address atomics: one per wave serialised 32 k atomics per launch
    // and tripled the kernels' time): dQ kernel at q8part[4·block + wave], dK/dV kernel at q8part2[...]
    float* q8part;
    float* q8part2;
};

// 4 values of a gradient row as e5m2 (one 4-B store) with the delayed scale, their amax folded into m
RN_DEV void attn_q8_store4(uint8_t* dst, float a, float b, float c, float d, float inv, float& m) {
    m = fmaxf(m, fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d))));
    const float lim = 57344.f;
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_bf8_f32(fminf(fmaxf(a * inv, -lim), lim), fminf(fmaxf(b * inv, -lim), lim), w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(fminf(fmaxf(c * inv, -lim), lim), fminf(fmaxf(d * inv, -lim), lim), w, true);
    *reinterpret_cast<int*>(dst) = w;
}
RN_DEV void attn_q8_amax(float* part, float m) {
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[blockIdx.x * 4 + (threadIdx.x >> 6)] = m;
}

// (bh, block) of this workgroup; `reverse`: the head's heaviest (last) causal block first
RN_DEV void blk_map(const AttnArgs& p, int nblk, bool reverse, int& bh, int& blk) {
    // head-interleaved 1-D grid of B·H·nblk blocks: block L works on head L % (B·H), so the
    // heaviest causal blocks of every head are dispatched first
    const int BH = p.B * p.H, L = blockIdx.x;
    const int i = L / BH;
    bh = L % BH;
    blk = reverse ? nblk - 1 - i : i;
}

// LDS tile geometry for head size D ∈ {32, 64, 128}: [64 rows][D bf16] = RB-byte rows, 16-B chunks
// XOR-swizzled per row.  Each swizzle is a permutation of the row's chunks that (a) makes the
// 16 rows of a ds_read_b128 row fragment (same logical chunk) land in 16 distinct 16-B bank slots
// and (b) keeps the 32-B chunk pairs of a ds_read_b64_tr_b16 column fragment (8 rows per pass) in
// 8 distinct 32-B slots; all three repeat with period 16 in the row, which FragOff relies on.
//   D = 64  (128-B rows, 2 per bank line): c ^ (((r>>1)&3)<<1)
//   D = 128 (256-B rows):                  c ^ (((r&7)<<1) | ((r>>3)&1))
//   D = 32  (64-B rows, 4 per bank line):  c ^ ((((r>>2)&1)<<1) | ((r>>3)&1))
template <int D = 64>
RN_DEV int swz(int r) {
    if constexpr (D == 64) return ((r >> 1) & 3) << 1;
    else if constexpr (D == 128) return ((r & 7) << 1) | ((r >> 3) & 1);
    else return (((r >> 2) & 1) << 1) | ((r >> 3) & 1);
}
template <int D> constexpr int kRB = 2 * D;        // bytes per tile row
template <int D> constexpr int kTB = 64 * 2 * D;   // bytes per 64-row tile
template <int D> constexpr int kNS = D / 32;       // 32-wide k-steps over the head dim
template <int D> constexpr int kNJ = D / 16;       // 16-wide output column blocks over the head dim

// Sum a wave-tile's [16 rows][D cols] accumulator (lane holds row lane&15, cols 16jd+4g+r)
// over the 64 rows of the 4 waves via LDS and write one partial row: out[col].
template <int D = 64>
RN_DEV void block_colsum64(const f32x4 (&acc)[kNJ<D>], float mul, float* lds, float* out, int wave, int lane) {
    const int g = lane >> 4, c = lane & 15;
    __syncthreads();  // LDS tiles no longer read by any wave
#pragma unroll
    for (int jd = 0; jd < kNJ<D>; ++jd)
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[(wave * 16 + c) * (D + 1) + jd * 16 + 4 * g + r] = acc[jd][r] * mul;
    __syncthreads();
    if (threadIdx.x < D) {
        float t = 0.f;
        for (int row = 0; row < 64; ++row) t += lds[row * (D + 1) + threadIdx.x];
        out[threadIdx.x] = t;
    }
}

// Per-lane parts of the rowfrag / colfrag LDS addresses, computed once per kernel.  Every call
// site reads row X*16 + (lane&15) (rowfrag) or rows 32*ks + … / columns 16*jd + … (colfrag) with
// X, ks, jd compile-time: the XOR swizzle then depends on the lane only, so the address is
// base + per-lane offset + an immediate, instead of ~50 recomputed VALU address ops per tile.
template <int D = 64>
struct FragOffT {
    uint32_t rf[kNS<D>];  // rowfrag, k-step s
    uint32_t cf[kNJ<D>];  // colfrag, column block jd
};
using FragOff = FragOffT<64>;
template <int D = 64>
RN_DEV FragOffT<D> make_fragoff(int lane) {
    FragOffT<D> f;
    const int g = lane >> 4, c = lane & 15;
    const int swc = swz<D>(c);
#pragma unroll
    for (int s = 0; s < kNS<D>; ++s) f.rf[s] = c * kRB<D> + ((((4 * s) + g) ^ swc) << 4);
    const int qq = c >> 2, pp = c & 3;
    const int r0 = 4 * g + qq;
    const int swr = swz<D>(r0);
#pragma unroll
    for (int jd = 0; jd < kNJ<D>; ++jd) f.cf[jd] = r0 * kRB<D> + (((2 * jd + (pp >> 1)) ^ swr) << 4) + (pp & 1) * 8;
    return f;
}
// == rowfrag<D>(t, X * 16 + (lane & 15), s, lane)
template <int D>
RN_DEV s16x8 rowfragx(const char* t, int X, int s, const FragOffT<D>& f) {
    return *reinterpret_cast<const s16x8*>(t + X * 16 * kRB<D> + f.rf[s]);
}
// == colfrag<D>(t, 32 * ks, 16 * jd, lane)
template <int D>
RN_DEV s16x8 colfragx(const char* t, int ks, int jd, const FragOffT<D>& f) {
    const char* a0 = t + ks * 32 * kRB<D> + f.cf[jd];
    s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
    s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + 16 * kRB<D>));
    s16x8 r;
    r[0] = v0[0]; r[1] = v0[1]; r[2] = v0[2]; r[3] = v0[3];
    r[4] = v1[0]; r[5] = v1[1]; r[6] = v1[2]; r[7] = v1[3];
    return r;
}

RN_DEV s16x8 gload16(const bf16* p, bool ok) {
    if (!ok) return (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
    return *reinterpret_cast<const s16x8*>(p);
}

RN_DEV short bfbits(float f) { return __builtin_bit_cast(short, (bf16)f); }

RN_DEV s16x8 pack_p(const f32x4& a, const f32x4& b) {
    s16x8 r;
    r[0] = bfbits(a[0]); r[1] = bfbits(a[1]); r[2] = bfbits(a[2]); r[3] = bfbits(a[3]);
    r[4] = bfbits(b[0]); r[5] = bfbits(b[1]); r[6] = bfbits(b[2]); r[7] = bfbits(b[3]);
    return r;
}

RN_DEV uint64_t drop_idx(const AttnArgs& p, int b, int h, int qi, int kj) {
    return (((uint64_t)(b * p.H + h) * p.Tq + qi) * (uint64_t)p.Tk) + kj;
}

#define MFMA __builtin_amdgcn_mfma_f32_16x16x32_bf16

// LDS-DMA issued through inline asm: the compiler then does not know a DMA is in
// flight, so it does not drain it (s_waitcnt vmcnt(0)) in front of every LDS read
// of the OTHER buffer — hipcc (ROCm 7.2) cannot tell the two buffers apart.  The
// hand-off is explicit instead: `s_waitcnt vmcnt(0)` + barrier at the top of each
// tile.  M0 (the DMA's LDS base) is written here; nothing else in these kernels
// uses it.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

RN_DEV u32x4 make_rsrc_sgpr(const void* base, uint32_t bytes = 0x7FFFFFF0u) {
    const uint64_t bp = (uint64_t)base;
    u32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((uint32_t)bp);
    r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(bp >> 32));
    r[2] = __builtin_amdgcn_readfirstlane(bytes);  // range-checked: dwords past it read as 0
    r[3] = 0x00020000u;
    return r;
}

RN_DEV uint32_t lds_addr(const char* p) {
    return __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void*)p);
}

#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"  // m0 is "reserved": declaring the clobber is still right
RN_DEV void dma16_async(const u32x4& rs_, uint32_t voff, uint32_t lds) {
    // re-assert uniformity: after the loop unrolling the divergence analysis can lose track of the
    // (readfirstlane-built) descriptor and hand the "s" constraint a VGPR tuple
    u32x4 rs;
#pragma unroll
    for (int i = 0; i < 4; ++i) rs[i] = __builtin_amdgcn_readfirstlane(rs_[i]);
    asm volatile("s_mov_b32 m0, %2\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(rs),
                 "s"(__builtin_amdgcn_readfirstlane(lds))
                 : "memory", "m0");
}
#pragma clang diagnostic pop

// Stage rows [r0, r0+64) (valid < rlim) of a [T][stride] bf16 matrix (D cols at the resource's
// base) into a swizzled LDS tile, by compiler-invisible LDS-DMA: D/8 16-B instructions in all,
// D/32 per wave; instruction `ins` fills rows ins·(512/D) .. +512/D (1 KiB of LDS).
template <int D = 64>
RN_DEV void stage64_async(const u32x4& rs, long st, int r0, int rlim, const char* lds, int wave, int lane) {
    constexpr int CPR = D / 8, RPI = 64 / CPR;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
        const int ins = wave * (D / 32) + i;
        const int r = ins * RPI + lane / CPR;
        const int cg = (lane % CPR) ^ swz<D>(r);
        const bool ok = (r0 + r) < rlim;
        const uint32_t voff = ok ? (uint32_t)((((long)(r0 + r)) * st + cg * 8) * 2) : 0xFFFFFFF0u;
        dma16_async(rs, voff, lds_addr(lds + ins * 1024));
    }
}

RN_DEV void vm_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// max over lanes {l, l^16, l^32, l^48} (the 4 lane groups holding one softmax row)
// with the gfx950 permlane swaps (VALU) instead of two ds_bpermute round trips.
RN_DEV float max4groups(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
RN_DEV float sum4groups(float x) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// ------------------------------------ host side ------------------------------------
constexpr int RES_T = 256;  // whole-head-resident kernels: Tq, Tk <= RES_T

// The kernel family that serves a call; attn_select (attention.hip) is the one place that decides it.
enum class AttnPath { Generic, Mfma, Resident, Causal8, Plain, BiasDrop };

// rn_attn_fwd / rn_attn_bwd return codes below the shape errors (-1 .. -3)
constexpr int ATTN_ERR_LAUNCH = -10;  // the launch itself failed
constexpr int ATTN_ERR_LDS = -11;     // the opt-in to more than 64 KiB of dynamic LDS was refused
constexpr int ATTN_ERR_PATH = -12;    // a <CAUSAL, BIAS, DROP> form the selection never asks for

// Every attention kernel is launched here (attention.hip).  A kernel that needs more than 64 KiB of dynamic
// LDS is opted in once per (kernel, device); returns 0, or ATTN_ERR_LDS / ATTN_ERR_LAUNCH.
int attn_launch(const void* kern, dim3 grid, int block, size_t lds, const AttnArgs& a, hipStream_t st);
int attn_cu_count();  // compute units of the current device (cached per device)

// Launch kern(CAUSAL, BIAS, DROP) — a generic lambda returning the kernel instance for three
// std::bool_constant tags — for the call's causal / bias / dropout combination.  PLAIN = false leaves the
// two <*, false, false> instances out of the table (never compiled): D = 64 serves that case elsewhere.
template <bool PLAIN, class K>
int attn_launch3(K kern, const AttnArgs& a, unsigned wgs, size_t lds, hipStream_t st) {
    using T = std::true_type;
    using F = std::false_type;
    const void* plain[2] = {nullptr, nullptr};
    if constexpr (PLAIN) {
        plain[0] = kern(F{}, F{}, F{});
        plain[1] = kern(T{}, F{}, F{});
    }
    const void* const tab[8] = {plain[0], kern(F{}, F{}, T{}), kern(F{}, T{}, F{}), kern(F{}, T{}, T{}),
                                plain[1], kern(T{}, F{}, T{}), kern(T{}, T{}, F{}), kern(T{}, T{}, T{})};
    const void* k = tab[(a.causal ? 4 : 0) + (a.bias ? 2 : 0) + (a.p_drop > 0.f ? 1 : 0)];
    return k ? attn_launch(k, dim3(wgs), 256, lds, a, st) : ATTN_ERR_PATH;
}

// Each unit's kernels behind plain functions; `wgs` is the workgroup count attn_select computed.
int attn_launch_fwd16(const AttnArgs& a, AttnPath path, unsigned wgs, hipStream_t st);     // attention_fwd.hip
int attn_launch_fwd32(const AttnArgs& a, AttnPath path, unsigned wgs, hipStream_t st);     // attention_mfma32.hip
int attn_launch_bwd_resident(const AttnArgs& a, hipStream_t st);                           // attention_mfma32.hip
// groups: 64-row groups per wave (1, or 2 at D = 64 without bias / dropout)
int attn_launch_dq_d32(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st);       // attention_dq_d32.hip
int attn_launch_dq_d64(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st);       // attention_dq_d64.hip
int attn_launch_dq_d128(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st);      // attention_dq_d128.hip
int attn_launch_dkdv_d32(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st);     // attention_dkdv_d32.hip
int attn_launch_dkdv_d64(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st);     // attention_dkdv_d64.hip
int attn_launch_dkdv_d128(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st);    // attention_dkdv_d128.hip
int attn_launch_fwd_generic(const AttnArgs& a, hipStream_t st);                            // attention_generic.hip
int attn_launch_bwd_generic(const AttnArgs& a, hipStream_t st);                            // attention_generic.hip

}  // namespace rn_attn
