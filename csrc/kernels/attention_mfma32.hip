// D = 64 on v_mfma_f32_32x32x16_bf16 (round 6): the forward attn_fwd32_k — causal streaming with 8 waves
// per workgroup, and whole-head-resident for Tq, Tk <= RES_T — and the whole-head-resident persistent
// backward attn_bwd_res_k.
//
// The causal forward re-tiled for the 32×32×16 MFMA.  Why: the 16×16×32 kernels (attention_fwd.hip) run with the
// softmax VALU beside their MFMAs, and a 16×16×32 MFMA holds the SIMD's vector issue for 8 of its 16
// cycles while a 32×32×16 one holds it for 8 of 32 (MI355X_MICROARCH.md, 'vector-instruction ISSUE
// cost'): for the same FLOPs the larger shape issues half the MFMA instructions and leaves 3× the issue
// cycles between them.
//   * the softmax row (the query) is the accumulator COLUMN (lane & 31), the keys sit in the 16
//     accumulator registers: a 32×32 result is the next MFMA's B operand after pairwise bf16 packing
//     (registers 8s'..8s'+7 = k-step s', element j of lane half h = row 16s' + 8(j>>2) + 4h + (j&3):
//     cdna_hip_programming.md §3), and V's column read (ds_read_b64_tr_b16 from the row-major LDS tile)
//     takes the same rows, so P never crosses lanes or LDS; a row max is 16 v_max3 + one permlane32 swap;
//   * LDS tiles [64 rows][64 bf16], 16-B chunk c of row r at c ^ swz32(r): conflict-free for the
//     32×32×16 row fragments (ds_read_b128 lane groups of the §LDS table) AND the transposed fragments
//     (4 consecutive rows × 4 chunks per 32-lane half); one image serves both (SQ_LDS_BANK_CONFLICT 0);
//   * row sums from a P·1 MFMA, the O rescale deferred until a row max grows past 2^8 (T13), mask work
//     only on the 32-key blocks the diagonal / Tk tail cuts.
// Measured (profiles/attention_r6.txt, GPT-2-small b64 causal): forward 0.187 -> 0.179 ms per layer.  The
// same re-tiling of dQ and dK/dV (with the dP accumulators started at −δ straight from LDS) was built,
// fp32-tested and measured SLOWER (0.559 -> 0.594 ms: dQ 238 -> 258 us, dK/dV 347 -> 352 us; MFMA busy
// 0.31-0.32 either way, 254 VGPRs in dK/dV); as the non-causal ViT forward (T = 197: 0.205 -> 0.212 ms)
// — both removed.  A software-pipelined dK/dV (query block 1's S / dP MFMAs issued before block 0's softmax
// VALU, block 0's dV / dK before block 1's; 246 VGPRs) closed half the gap (+2 %), sched_group_barrier
// interleaving of those phases nothing more, occupancy 1 (122 VGPR + 160 AGPR) lost 33 %: removed too.  Their unmasked loops were already lean (per 32 MFMAs: 32 fma / exp / mul / cvt_pk),
// so the remaining gap is stall structure (WAIT_ANY ≈ 0.3-0.4), not instruction count.
#include "attention_common.h"

#include <algorithm>

namespace rn_attn {
namespace {

typedef __attribute__((address_space(3))) const s16x8 lds_s16x8;
typedef __attribute__((address_space(3))) const f32x4 lds_f32x4;
#define MFMA32 __builtin_amdgcn_mfma_f32_32x32x16_bf16

RN_DEV int swz32(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }

// per-lane LDS offsets of the 32×32×16 fragments in a swz32 tile (rows of a 32-row block r0 = 32·X):
//   row fragment (A operand, row r0 + (lane&31), k-step s = columns 16s + 8h .. +7): rf[s]
//   transposed fragment (A operand, row = column 32·jd + (lane&31) of the tile, k-step rows
//   r0 + 16s' + 8(j>>2) + 4h + (j&3)): two ds_read_b64_tr_b16 at cf[jd][0] / cf[jd][1]
struct Frag32 {
    uint32_t rf[4];
    uint32_t cf[2][2];
};
RN_DEV Frag32 make_frag32(int lane) {
    Frag32 f;
    const int r = lane & 31, h = lane >> 5;
    const int sw = swz32(r);
#pragma unroll
    for (int s = 0; s < 4; ++s) f.rf[s] = r * 128 + (((2 * s + h) ^ sw) << 4);
    const int i = lane & 15, qq = i >> 2, pp = i & 3, gp = (lane >> 4) & 1;
#pragma unroll
    for (int jd = 0; jd < 2; ++jd)
#pragma unroll
        for (int sec = 0; sec < 2; ++sec) {
            const int R = 4 * h + qq + 8 * sec;
            const int ch = 4 * jd + 2 * gp + (pp >> 1);
            f.cf[jd][sec] = R * 128 + ((ch ^ swz32(R)) << 4) + (pp & 1) * 8;
        }
    return f;
}
// row fragment of 32-row block X, k-step s
RN_DEV s16x8 rfrag32(const char* t, int X, int s, const Frag32& f) {
    return *reinterpret_cast<const s16x8*>(t + X * 32 * 128 + f.rf[s]);
}
// transposed fragment: tile rows 16·ks + … (ks = 0..3 over the 64-row tile), tile columns 32·jd + (lane&31)
RN_DEV s16x8 tfrag32(const char* t, int ks, int jd, const Frag32& f) {
    const char* a = t + ks * 16 * 128;
    s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + f.cf[jd][0]));
    s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + f.cf[jd][1]));
    s16x8 r;
    r[0] = v0[0]; r[1] = v0[1]; r[2] = v0[2]; r[3] = v0[3];
    r[4] = v1[0]; r[5] = v1[1]; r[6] = v1[2]; r[7] = v1[3];
    return r;
}
// registers 8s'..8s'+7 of a 32×32 accumulator as a bf16 B-operand fragment (k-step s')
RN_DEV s16x8 pack16(const f32x16& x, int s2) {
    s16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = bfbits(x[8 * s2 + j]);
    return r;
}
RN_DEV float swap_max(float x) {
    auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
}
RN_DEV float swap_sum(float x) {
    auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}
// accumulator row of register i for lane half h
RN_DEV constexpr int arow(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// store a wave's [64 d][32 cols] accumulator pair as rows (col = this lane's row of the output):
// out[d] = x·mul in bf16 (and, q8, e5m2 of the bf16 value with the delayed scale)
RN_DEV void store_rows32(const f32x16 (&x)[2], float mul, bf16* dst, uint8_t* q8dst, bool bf, float q8inv, float& q8m,
                         int h) {
#pragma unroll
    for (int jd = 0; jd < 2; ++jd)
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
            const int d = 32 * jd + 8 * c4 + 4 * h;
            const bf16x4 v = {(bf16)(x[jd][4 * c4] * mul), (bf16)(x[jd][4 * c4 + 1] * mul), (bf16)(x[jd][4 * c4 + 2] * mul),
                              (bf16)(x[jd][4 * c4 + 3] * mul)};
            if (q8dst) attn_q8_store4(q8dst + d, (float)v[0], (float)v[1], (float)v[2], (float)v[3], q8inv, q8m);
            if (bf) *reinterpret_cast<bf16x4*>(dst + d) = v;
        }
}

// ---------------- forward: 8 waves × 32 queries, 64-key tiles ----------------
// RES (Tq, Tk <= 256, RES_T): one workgroup of 8 waves per (b, h) holds the head's whole K and V in LDS
// (staged once, 64 KiB, no barrier inside the key loop): K / V are read from HBM once per head instead
// of once per 128-query block.  At ViT-B/16's T = 197 the streaming kernel reads K and V twice and
// the forward is HBM-bound (Q + 2K + 2V + O per layer).
// Streaming (!RES, causal only): 8 waves × 32 queries per workgroup, not 4: every staged K / V tile serves 256
// queries, so a causal head fetches its K / V tiles 40 times instead of 72 (T = 1024).
template <bool CAUSAL, bool RES>
__global__ void __launch_bounds__(512, 4) attn_fwd32_k(AttnArgs p) {
    static_assert(CAUSAL || RES, "the non-causal streaming forward is attn_fwd64v2_k");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Frag32 fo = make_frag32(lane);
    constexpr int QB = 256;  // queries per workgroup
    int bh, qb;
    if constexpr (RES) {
        bh = blockIdx.x;
        qb = 0;
    } else {
        blk_map(p, (p.Tq + QB - 1) / QB, CAUSAL, bh, qb);
    }
    const int b = bh / p.H, hh = bh % p.H;
    const int q0 = qb * QB + wave * 32;  // this wave's first query
    const int qg = q0 + r;               // this lane's query
    const int off = p.Tk - p.Tq;
    const float sl2 = p.scale * LOG2E;
    const bf16* qbase = p.q + b * p.q_sb + hh * p.q_sh;
    const u32x4 krs = make_rsrc_sgpr(p.k + b * p.k_sb + hh * p.k_sh);
    const u32x4 vrs = make_rsrc_sgpr(p.v + b * p.v_sb + hh * p.v_sh);
    int kv_end = p.Tk;
    if (CAUSAL) kv_end = min(p.Tk, qb * QB + QB + off);
    const int nkv = kv_end > 0 ? (kv_end + 63) / 64 : 0;
    int nfull = p.Tk / 64;  // tiles every key of which every query of the block sees
    if (CAUSAL) nfull = min(nfull, max(0, (qb * QB + off + 1) / 64));
    nfull = min(nfull, nkv);
    // streaming: double-buffered [K 64 rows | V 64 rows] pairs; RES: K rows [0, 256) then V rows [0, 256)
#define Kt(i) (RES ? smem + (i) * 8192 : smem + ((i) & 1) * 16384)
#define Vt(i) (RES ? smem + 32768 + (i) * 8192 : smem + 8192 + ((i) & 1) * 16384)
    // one 64-row K tile and V tile (streaming): each of the 8 waves issues 1 piece of each
    auto stage_kv = [&](int t) {
        const int row = wave * 8 + (lane >> 3);
        const int cg = (lane & 7) ^ swz32(row);
        const bool ok = t * 64 + row < p.Tk;
        dma16_async(krs, ok ? (uint32_t)((((long)(t * 64 + row)) * p.k_st + cg * 8) * 2) : 0xFFFFFFF0u,
                    lds_addr(Kt(t) + wave * 1024));
        dma16_async(vrs, ok ? (uint32_t)((((long)(t * 64 + row)) * p.v_st + cg * 8) * 2) : 0xFFFFFFF0u,
                    lds_addr(Vt(t) + wave * 1024));
    };
    if constexpr (RES) {
        // every 8-row piece of the nkv tiles (rows past Tk read as zeros: V's padding rows must be finite)
        for (int ins = wave; ins < nkv * 8; ins += 8) {
            const int row = ins * 8 + (lane >> 3);
            const int cg = (lane & 7) ^ swz32(row);
            const bool ok = row < p.Tk;
            dma16_async(krs, ok ? (uint32_t)(((long)row * p.k_st + cg * 8) * 2) : 0xFFFFFFF0u, lds_addr(smem + ins * 1024));
            dma16_async(vrs, ok ? (uint32_t)(((long)row * p.v_st + cg * 8) * 2) : 0xFFFFFFF0u,
                        lds_addr(smem + 32768 + ins * 1024));
        }
    } else if (nkv > 0) {
        stage_kv(0);
    }
    s16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = gload16(qbase + (long)qg * p.q_st + 16 * s + 8 * h, qg < p.Tq);
#pragma unroll
    for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(qf[s]));
    // Online softmax in log2 units (ms = running row max × sl2) with a deferred rescale (cdna_hip_programming.md
    // T13): O and the row sum are rescaled only when some row's tile max exceeds ms by more than THR, so p ≤
    // 2^THR (exact in fp32, the usual relative error in the bf16 P operand).  Row sums come from a P·1 MFMA
    // (every register of lsum holds the running sum of its column; [0] is read): 2 MFMAs per 32 keys
    // instead of 32 adds, the VALU being this kernel's bound (PMC, profiles/attention_r6f.txt).
    constexpr float THR = 8.f;
    float ms = -INFINITY;
    f32x16 oacc[2], lsum;
#pragma unroll
    for (int i = 0; i < 16; ++i) { oacc[0][i] = 0.f; oacc[1][i] = 0.f; lsum[i] = 0.f; }
    const short one = 0x3F80;  // bf16 1.0
    const s16x8 ones = {one, one, one, one, one, one, one, one};

    auto tile = [&](const int t, auto masked_c) {
        constexpr bool MASKED = decltype(masked_c)::value;
        const char* kt = Kt(t);
        const char* vt = Vt(t);
        const int kv0 = t * 64;
        // 32-key block class (wave-uniform): 0 dead (past Tk / above every query of this wave), 1 every key
        // visible to every query, 2 partial (the causal diagonal, the ragged Tk tail): per-element mask
        auto cls = [&](int kb) -> int {
            if constexpr (!MASKED) return 1;
            const int k0 = kv0 + 32 * kb;
            if (k0 >= p.Tk) return 0;
            if (CAUSAL && k0 > min(q0 + 31, p.Tq - 1) + off) return 0;
            return (k0 + 31 >= p.Tk || (CAUSAL && k0 + 31 > q0 + off)) ? 2 : 1;
        };
        f32x16 sacc[2];
        float pm = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            const int c_ = cls(kb);
            if (MASKED && c_ == 0) continue;
            f32x16 a;
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) a = MFMA32(rfrag32(kt, kb, s, fo), qf[s], a, 0, 0, 0);
            if (MASKED && c_ == 2) {
                const int lim = CAUSAL ? min(qg + off, p.Tk - 1) : p.Tk - 1;
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (kv0 + 32 * kb + arow(i, h) > lim) a[i] = -INFINITY;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) pm = fmaxf(pm, a[i]);
            sacc[kb] = a;
        }
        pm = swap_max(pm) * sl2;
        if (__builtin_amdgcn_ballot_w64(pm > ms + THR)) {  // wave-uniform, rare after the first tile
            const float mn = fmaxf(ms, pm);
            const float alpha = (ms == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(ms - mn);
            oacc[0] *= alpha;
            oacc[1] *= alpha;
            lsum[0] *= alpha;
            ms = mn;
        }
        // (masked tiles: a row with no visible key so far keeps ms = -inf and p = 0)
        const float nms = (MASKED && ms == -INFINITY) ? 0.f : -ms;
        // O^T[d][q] += V^T[d][key] P^T[key][q];  lsum += 1 · P^T
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            if (MASKED && cls(kb) == 0) continue;
#pragma unroll
            for (int i = 0; i < 16; ++i) sacc[kb][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[kb][i], sl2, nms));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const s16x8 pb = pack16(sacc[kb], s2);
#pragma unroll
                for (int jd = 0; jd < 2; ++jd) oacc[jd] = MFMA32(tfrag32(vt, 2 * kb + s2, jd, fo), pb, oacc[jd], 0, 0, 0);
                lsum = MFMA32(ones, pb, lsum, 0, 0, 0);
            }
        }
    };
    auto sync_prefetch = [&](int t) {
        if constexpr (RES) {
            if (t == 0) {
                vm_wait_all();
                __syncthreads();
            }
            return;
        }
        vm_wait_all();
        __syncthreads();
        if (t + 1 < nkv) stage_kv(t + 1);
    };
    const int nf = q0 < p.Tq ? nfull : 0;
    int t = 0;
    for (; t < nf; ++t) {
        sync_prefetch(t);
        tile(t, std::false_type{});
    }
    for (; t < nkv; ++t) {
        sync_prefetch(t);
        if (CAUSAL && t * 64 > q0 + 31 + off) continue;  // wave-uniform: every query precedes the tile
        if (q0 >= p.Tq) continue;
        tile(t, std::true_type{});
    }
#undef Kt
#undef Vt
    const float lt = lsum[0];  // (the full sum over both lane halves' keys: the MFMA summed them)
    if (qg < p.Tq) {
        const float inv = lt > 0.f ? 1.f / lt : 0.f;
        float dummy = 0.f;
        store_rows32(oacc, inv, p.o + b * p.o_sb + (long)qg * p.o_st + hh * p.o_sh, nullptr, true, 0.f, dummy, h);
        if (h == 0) p.lse[((long)b * p.H + hh) * p.Tq + qg] = (lt > 0.f) ? (ms + log2f(lt)) : INFINITY;
    }
}

// ---------------- backward, whole head resident (Tq, Tk <= RES_T; non-causal, no bias / dropout / e5m2) ----------------
// ViT-B/16 (T = 197) is HBM-bound in the streaming backward: the dQ kernel re-reads K / V per 128-query
// block, the dK/dV kernel Q / dO per 128-key block, and δ makes a round trip.  Here one persistent 8-wave
// workgroup per CU walks the heads; a head's Q, dO, K, V tiles sit in LDS (128 KiB) and every operand is read
// from HBM once:
//   A   δ of the wave's 32 queries (O rows in registers · dO rows of the tile); lse, −δ -> LDS   (barrier B0)
//   P1  wave w owns keys [32w, 32w+32): K / V rows in registers (loaded at the end of the previous head),
//       loops over every query block of the Q / dO tiles: S, dP, P, dS; dV^T += dO^T P, dK^T += Q^T dS (B1)
//       -> the Q / dO tiles of the NEXT head stream in during P2
//   P2  wave w owns queries [32w, 32w+32): loops over every key block from the K / V tiles:
//       S^T, dP^T, dS^T; dQ^T += K^T dS^T                                             (barrier B2)
//       -> the K / V tiles of the next head stream in during the next A + P1
// The 32×32×16 orientation and fragment helpers are the forward's (accumulator column = the row that
// owns the result, reduced index in registers).  Rows past Tq / Tk are zero-filled by the DMA and lse = +inf
// there, so only the ragged key block of P2 needs a mask.
// QKV bias partials (bsum): Σ_rows dV = Σ_q dO (softmax rows sum to 1; dO^T·1 on the MFMA), Σ_rows dK = 0 (a key
// bias shifts all of a query's scores alike), Σ_rows dQ by an in-register reduce-scatter of each wave's dQ^T —
// all written into the head's first 64-row block (the consumer sums every block).
constexpr int RES_LDS = 4 * 32768 + 2 * 1024 + 2 * 8 * 64 * 4;  // tiles, lse | −δ, bias partials
constexpr int RES_TILE_PIECES = 4;  // 16-B LDS-DMA pieces per wave per [256][64] tile: 32 8-row pieces over 8 waves
__global__ void __launch_bounds__(512, 2) attn_bwd_res_k(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Qt = smem;
    char* const Dt = smem + 32768;
    char* const Kt = smem + 65536;
    char* const Vt = smem + 98304;
    float* const lseL = reinterpret_cast<float*>(smem + 131072);  // [256] −lse / (scale·log2 e) (−inf past Tq)
    float* const ndL = lseL + 256;                                 // [256] −δ
    float* const bpL = ndL + 256;                                  // [2][8][64] bias partials: dQ, dV
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Frag32 fo = make_frag32(lane);
    const float sl2 = p.scale * LOG2E;
    const int BH = p.B * p.H, E = p.H * 64;
    const int nqb = (p.Tq + 31) / 32, nkb = (p.Tk + 31) / 32;
    const int w0 = wave * 32;  // this wave's keys (P1) and queries (P2)
    const short one = 0x3F80;
    const s16x8 ones = {one, one, one, one, one, one, one, one};

    s16x8 kf[4], vf[4], orw[4];
    float lsel;
    // registers of head bh: K / V rows w0 + r (P1's B operands), O rows w0 + r (δ), lse
    auto issue_regs = [&](int bh) {
        const int b = bh / p.H, hh = bh % p.H;
        int row = w0 + r;
        asm volatile("" : "+v"(row));  // (as in issue_tiles)
        const bool kok = row < p.Tk, qok = row < p.Tq;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c = 16 * s + 8 * h;
            kf[s] = gload16(p.k + b * p.k_sb + (long)row * p.k_st + hh * p.k_sh + c, kok);
            vf[s] = gload16(p.v + b * p.v_sb + (long)row * p.v_st + hh * p.v_sh + c, kok);
            orw[s] = gload16(p.o + b * p.o_sb + (long)row * p.o_st + hh * p.o_sh + c, qok);
        }
        lsel = qok ? p.lse[((long)b * p.H + hh) * p.Tq + row] : INFINITY;
    };
    // two [256][64] tiles by LDS-DMA, RES_TILE_PIECES of each per wave whatever T (rows past `lim` zero-filled):
    // the K / V pair must be this wave's 2·RES_TILE_PIECES youngest loads (the s_waitcnt vmcnt below)
    auto issue_tiles = [&](const bf16* x0, long st0, const bf16* x1, long st1, int lim, char* t0, char* t1) {
        const u32x4 rs0 = make_rsrc_sgpr(x0), rs1 = make_rsrc_sgpr(x1);
#pragma unroll
        for (int i = 0; i < RES_TILE_PIECES; ++i) {
            const int ins = wave + 8 * i;
            int row = ins * 8 + (lane >> 3);
            asm volatile("" : "+v"(row));  // recomputed per head: hoisted out of the head loop they were spilled
            const int cg = (lane & 7) ^ swz32(row);
            const bool ok = row < lim;
            dma16_async(rs0, ok ? (uint32_t)(((long)row * st0 + cg * 8) * 2) : 0xFFFFFFF0u, lds_addr(t0 + ins * 1024));
            dma16_async(rs1, ok ? (uint32_t)(((long)row * st1 + cg * 8) * 2) : 0xFFFFFFF0u, lds_addr(t1 + ins * 1024));
        }
    };
    auto issue_qdo = [&](int bh) {
        const int b = bh / p.H, hh = bh % p.H;
        issue_tiles(p.q + b * p.q_sb + hh * p.q_sh, p.q_st, p.dout + b * p.do_sb + hh * p.do_sh, p.do_st, p.Tq, Qt, Dt);
    };
    auto issue_kv = [&](int bh) {
        const int b = bh / p.H, hh = bh % p.H;
        issue_tiles(p.k + b * p.k_sb + hh * p.k_sh, p.k_st, p.v + b * p.v_sb + hh * p.v_sh, p.v_st, p.Tk, Kt, Vt);
    };

    // LDS byte addresses held whole in one register (opaque to the compiler, which otherwise re-adds the
    // >64 KiB tile bases — beyond ds_read's 16-bit offset — to every address in the loops); the block /
    // tile / dO-V offsets then ride the instructions' immediates
    auto la = [](const void* ptr, uint32_t off) -> uint32_t {
        uint32_t x = (uint32_t)(uintptr_t)(lds_void*)ptr + off;
        asm volatile("" : "+v"(x));
        return x;
    };
    auto ld16 = [](uint32_t a) -> s16x8 { return *reinterpret_cast<const lds_s16x8*>((size_t)a); };
    auto trd = [](uint32_t a0, uint32_t a1) -> s16x8 {  // a transposed fragment's two ds_read_b64_tr_b16
        const s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)a0);
        const s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(size_t)a1);
        return (s16x8){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    };
    auto ldf4 = [](uint32_t a) -> f32x4 { return *reinterpret_cast<const lds_f32x4*>((size_t)a); };

    int bh = blockIdx.x;
    if (bh < BH) {
        issue_qdo(bh);
        issue_regs(bh);
        issue_kv(bh);
    }
    for (; bh < BH; bh += gridDim.x) {
        const int b = bh / p.H, hh = bh % p.H;
        const int nxt = bh + gridDim.x;
        // ---- A ----
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * RES_TILE_PIECES) : "memory");  // everything but this head's K / V pieces
        __syncthreads();  // (every wave's Q / dO pieces)
        float dsum = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const s16x8 dr = rfrag32(Dt, wave, s, fo);  // dO row w0 + r, the columns orw[s] holds
#pragma unroll
            for (int j = 0; j < 8; ++j)
                dsum += __uint_as_float((uint32_t)(unsigned short)orw[s][j] << 16) *
                        __uint_as_float((uint32_t)(unsigned short)dr[j] << 16);
        }
        const float ndl = -swap_sum(dsum);  // −δ of query w0 + r (0 past Tq: zero rows)
        const float lse2 = lsel;
        if (h == 0) {
            lseL[w0 + r] = -lsel / sl2;  // P1 starts its S accumulators here: P = exp2(acc · sl2)
            ndL[w0 + r] = ndl;
        }
        __syncthreads();  // B0: lse, −δ
        if (p.bsum) {  // Σ_q dO[q][d] over this wave's 32 queries: dO^T · 1 on the MFMA (P1's dV product with P = 1)
            const Frag32 f2 = make_frag32(lane);
            f32x16 u[2];
#pragma unroll
            for (int i = 0; i < 16; ++i) { u[0][i] = 0.f; u[1][i] = 0.f; }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int jd = 0; jd < 2; ++jd) u[jd] = MFMA32(tfrag32(Dt, 2 * wave + s2, jd, f2), ones, u[jd], 0, 0, 0);
            if (r == 0) {  // every column of u holds the sums: lanes 0 / 32 write rows arow(i, h)
#pragma unroll
                for (int jd = 0; jd < 2; ++jd)
#pragma unroll
                    for (int i = 0; i < 16; ++i) bpL[512 + wave * 64 + 32 * jd + arow(i, h)] = u[jd][i];
            }
        }
        // ---- P1: dK, dV of keys w0 .. w0+31 ----
        f32x16 dk[2], dv[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) { dk[0][i] = dk[1][i] = dv[0][i] = dv[1][i] = 0.f; }
        if (w0 < p.Tk) {
            // per-lane LDS pointers into the Q tile (dO: +32768, block X: +4096·X — immediates / one add each)
            uint32_t qr[4], qc[2][2];
#pragma unroll
            for (int s = 0; s < 4; ++s) qr[s] = la(Qt, fo.rf[s]);
#pragma unroll
            for (int jd = 0; jd < 2; ++jd) {
                qc[jd][0] = la(Qt, fo.cf[jd][0]);
                qc[jd][1] = la(Qt, fo.cf[jd][1]);
            }
            const uint32_t nda = la(ndL, 16 * h), lsa = la(lseL, 16 * h);
            s16x8 qa[4], da[4];
#pragma unroll 1
            for (int X = 0; X < nqb; ++X) {
                const int xo = X * 4096;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    qa[s] = ld16(qr[s] + xo);
                    da[s] = ld16(qr[s] + xo + 32768);
                }
                f32x16 sa, dp;
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const f32x4 nd = ldf4(nda + 128 * X + 32 * c4);
                    const f32x4 nl = ldf4(lsa + 128 * X + 32 * c4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { dp[4 * c4 + e] = nd[e]; sa[4 * c4 + e] = nl[e]; }
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) sa = MFMA32(qa[s], kf[s], sa, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < 4; ++s) dp = MFMA32(da[s], vf[s], dp, 0, 0, 0);
                // dO^T / Q^T fragments of the dV / dK products read now: their latency hides under the softmax VALU
                s16x8 to[2][2], tq[2][2];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                    for (int jd = 0; jd < 2; ++jd) {
                        const int o = xo + s2 * 2048;
                        to[s2][jd] = trd(qc[jd][0] + o + 32768, qc[jd][1] + o + 32768);
                        tq[s2][jd] = trd(qc[jd][0] + o, qc[jd][1] + o);
                    }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    sa[i] = __builtin_amdgcn_exp2f(sa[i] * sl2);  // P
                    dp[i] *= sa[i];                               // dS
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const s16x8 pb = pack16(sa, s2);
#pragma unroll
                    for (int jd = 0; jd < 2; ++jd) dv[jd] = MFMA32(to[s2][jd], pb, dv[jd], 0, 0, 0);
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const s16x8 db = pack16(dp, s2);
#pragma unroll
                    for (int jd = 0; jd < 2; ++jd) dk[jd] = MFMA32(tq[s2][jd], db, dk[jd], 0, 0, 0);
                }
            }
        }
        // P2's B operands (Q / dO rows w0 + r) while the tiles are resident
        s16x8 qf[4], df[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qf[s] = rfrag32(Qt, wave, s, fo);
            df[s] = rfrag32(Dt, wave, s, fo);
        }
        vm_wait_all();  // this head's K / V tiles (issued before A)
        if (w0 + r < p.Tk) {
            float dummy = 0.f;
            store_rows32(dk, p.scale, p.dk + b * p.dk_sb + (long)(w0 + r) * p.dk_st + hh * p.dk_sh, nullptr, true, 0.f,
                         dummy, h);
            store_rows32(dv, 1.f, p.dv + b * p.dv_sb + (long)(w0 + r) * p.dv_st + hh * p.dv_sh, nullptr, true, 0.f,
                         dummy, h);
        }
        __syncthreads();  // B1: Q / dO tiles free; K / V tiles and Σ_q dS complete
        if (nxt < BH) {
            issue_qdo(nxt);
            issue_regs(nxt);
        }
        // ---- P2: dQ of queries w0 .. w0+31 ----
        f32x16 dq[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) { dq[0][i] = dq[1][i] = 0.f; }
        if (w0 < p.Tq) {
            uint32_t kr[4], kc[2][2];  // per-lane addresses in the K tile (V: +32768)
#pragma unroll
            for (int s = 0; s < 4; ++s) kr[s] = la(Kt, fo.rf[s]);
#pragma unroll
            for (int jd = 0; jd < 2; ++jd) {
                kc[jd][0] = la(Kt, fo.cf[jd][0]);
                kc[jd][1] = la(Kt, fo.cf[jd][1]);
            }
            s16x8 ka[4], va[4];
#pragma unroll 1
            for (int kb = 0; kb < nkb; ++kb) {
                const int ko = kb * 4096;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    ka[s] = ld16(kr[s] + ko);
                    va[s] = ld16(kr[s] + ko + 32768);
                }
                f32x16 sa, dp;
#pragma unroll
                for (int i = 0; i < 16; ++i) { sa[i] = 0.f; dp[i] = ndl; }
#pragma unroll
                for (int s = 0; s < 4; ++s) sa = MFMA32(ka[s], qf[s], sa, 0, 0, 0);
#pragma unroll
                for (int s = 0; s < 4; ++s) dp = MFMA32(va[s], df[s], dp, 0, 0, 0);
                // both chains issued before the softmax VALU (which then overlaps the dP chain); left alone the
                // scheduler put the dP MFMAs after the exps, exposing both chains' latency
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 16; ++i) sa[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(sa[i], sl2, -lse2));
                if (32 * kb + 32 > p.Tk) {  // the ragged key block (wave-uniform)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (32 * kb + arow(i, h) >= p.Tk) sa[i] = 0.f;
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) dp[i] *= sa[i];
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const s16x8 db = pack16(dp, s2);
                    const int o = ko + s2 * 2048;
#pragma unroll
                    for (int jd = 0; jd < 2; ++jd) dq[jd] = MFMA32(trd(kc[jd][0] + o, kc[jd][1] + o), db, dq[jd], 0, 0, 0);
                }
            }
        }
        if (w0 + r < p.Tq) {
            float dummy = 0.f;
            store_rows32(dq, p.scale, p.dq + b * p.dq_sb + (long)(w0 + r) * p.dq_st + hh * p.dq_sh, nullptr, true, 0.f,
                         dummy, h);
        }
        if (p.bsum) {
            // Σ_q dQ[q][d] over this wave's 32 queries: a reduce-scatter of the dQ^T accumulator across the 32
            // lanes of each half (5 levels of XOR partners; at each, a lane keeps the half of its values its
            // lane bit selects and adds the partner's copy of them), so lane r ends with value v = r: d = 32·(r>>4)
            // + arow(r & 15, h).  Rows past Tq hold zeros (P = 0 there).  No LDS round trip, no extra barrier.
            float cur[32];
#pragma unroll
            for (int v = 0; v < 32; ++v) cur[v] = dq[v >> 4][v & 15];
#pragma unroll
            for (int m = 16; m >= 1; m >>= 1) {
                const bool hi = (r & m) != 0;
#pragma unroll
                for (int k = 0; k < m; ++k) {
                    const float keep = hi ? cur[k + m] : cur[k];
                    const float send = hi ? cur[k] : cur[k + m];
                    cur[k] = keep + __shfl_xor(send, m, 64);
                }
            }
            bpL[wave * 64 + 32 * (r >> 4) + arow(r & 15, h)] = cur[0];
        }
        __syncthreads();  // B2: K / V tiles free, bias partials complete
        if (p.bsum && threadIdx.x < 128) {
            const int part = threadIdx.x >> 6, d = lane;  // 0: dQ (and dK), 1: dV
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) a += bpL[part * 512 + w * 64 + d];
            const int nb64 = (p.Tq + 63) / 64;
            float* row = p.bsum + (long)b * nb64 * 3 * E + hh * 64 + d;
            if (part == 0) {
                row[0] = a * p.scale;
                row[E] = 0.f;
            } else {
                row[2 * E] = a;
            }
            for (int blk = 1; blk < nb64; ++blk) {
                float* z = row + (long)blk * 3 * E;
                if (part == 0) {
                    z[0] = 0.f;
                    z[E] = 0.f;
                } else {
                    z[2 * E] = 0.f;
                }
            }
        }
        if (nxt < BH) issue_kv(nxt);  // the loop body's last vector-memory operation: vmcnt above counts on it
    }
}

#undef MFMA32

}  // namespace

int attn_launch_fwd32(const AttnArgs& a, AttnPath path, unsigned wgs, hipStream_t st) {
    if (a.D != 64 || a.bias || a.p_drop > 0.f) return ATTN_ERR_PATH;
    if (path == AttnPath::Resident) {  // one 8-wave workgroup per (b, h): K and V rows [0, 256) in 64 KiB
        const void* k = a.causal ? (const void*)attn_fwd32_k<true, true> : (const void*)attn_fwd32_k<false, true>;
        return attn_launch(k, dim3(wgs), 512, 65536, a, st);
    }
    if (path != AttnPath::Causal8 || !a.causal) return ATTN_ERR_PATH;
    return attn_launch((const void*)attn_fwd32_k<true, false>, dim3(wgs), 512, 32768, a, st);
}

// persistent over the CUs; ATTN_ERR_LDS when the device refuses the 137 KiB of LDS (the caller then
// runs the streaming dQ + dK/dV pair)
int attn_launch_bwd_resident(const AttnArgs& a, hipStream_t st) {
    if (a.D != 64 || a.causal || a.bias || a.p_drop > 0.f || a.q8 || a.Tq > RES_T || a.Tk > RES_T) return ATTN_ERR_PATH;
    return attn_launch((const void*)attn_bwd_res_k, dim3(std::min(a.B * a.H, attn_cu_count())), 512, RES_LDS, a, st);
}

}  // namespace rn_attn
