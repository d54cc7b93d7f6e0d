// Fused scaled-dot-product attention, forward + backward (N4/N5): the host entry points, the one place
// that chooses a kernel family (attn_select) and the one launch (attn_launch).  The kernels live in
//   attention_fwd.hip            forward on 16×16×32: single-loop (bias / dropout, D = 32 / 128), split-loop v2
//   attention_mfma32.hip         D = 64 on 32×32×16: causal 8-wave and whole-head-resident forward, resident backward
//   attention_dq_d{32,64,128}.hip, attention_dkdv_d{32,64,128}.hip
//                                streaming backward, instantiated per head size from attention_bwd_impl.h
//   attention_generic.hip        head sizes without an MFMA kernel
// with the shared device helpers and the launcher declarations in attention_common.h.
//
// Layout: q/k/v/o are [B][T][H][D] with arbitrary batch/token/head strides
// (q, k, v are usually views into one packed QKV GEMM output).  LSE is saved as
// [B][H][Tq] fp32 (base 2 from the MFMA kernels, natural log from the generic one: AttnArgs::lse_log2).
//
// MFMA path, head size D ∈ {32, 64, 128} (D = 64: GPT-2 small/medium, ViT-B/16; 32 / 128: the
// reference blocks' E // n_heads at e.g. 256/8 and 512/4), all v_mfma_f32_16x16x32_bf16:
//   * every product is arranged so that the softmax row index (the query for
//     fwd / dQ, the key for dK/dV) sits on lane&15 and the reduced index sits in
//     accumulator registers: the accumulator tile is then directly the next
//     MFMA's B operand (no LDS round trip, no lane shuffles for P or dS);
//     the k-order inside each 32-wide k-step is permuted identically on both
//     operands ({4g..4g+3} ∪ {16+4g..16+4g+3} for lane group g);
//   * the other operand of those products is a column slice of a row-major LDS
//     tile, read with ds_read_b64_tr_b16 (hardware transpose);
//   * LDS tiles are [64 rows][D bf16] staged by LDS-DMA (buffer_load … lds) with a
//     per-D 16-B chunk XOR swizzle (swz<D>) that is conflict-free for BOTH the
//     ds_read_b128 row reads and the transposed reads (one image serves both);
//   * online softmax in exp2 domain; causal tiles above the diagonal are
//     skipped, diagonal tiles masked; heaviest causal blocks launch first;
//   * dropout on P by a stateless counter hash, regenerated in the backward;
//   * backward = dQ kernel (one workgroup per 64 queries, loops over keys; also
//     emits delta = rowsum(dO·O) from registers) + dK/dV kernel (one workgroup
//     per 64 keys, loops over queries): no atomics, bitwise deterministic.
// D = 64 has extra tuned variants (split-loop forward with MFMA row sums, two query / key
// groups per wave in the backward); D = 32 / 128 use the single-loop forward and one group.
// Generic path (odd head sizes ≤ 256 only): per-query-row kernels with fp32 scores in LDS; the
// backward is dQ per query row, then dK/dV per key row (no atomics).
// Round 6 (D = 64): the 32×32×16 forward (causal: 8 waves / 256 queries per workgroup), and for
// Tq, Tk ≤ 256 whole-head-resident forward / backward kernels (docs/DESIGN.md §4 has the selection table).
#include "attention_common.h"
#include "rn_api.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

namespace rn_attn {

int attn_launch(const void* kern, dim3 grid, int block, size_t lds, const AttnArgs& a, hipStream_t st) {
    if (lds > 65536) {
        static std::mutex mu;
        // (kernel, device) -> {bytes opted in, smallest size the device refused (0: none)}
        static std::map<std::pair<const void*, int>, std::pair<size_t, size_t>> optin;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return ATTN_ERR_LAUNCH;
        std::lock_guard<std::mutex> lock(mu);
        auto& [have, refused] = optin[{kern, dev}];
        if (refused && lds >= refused) return ATTN_ERR_LDS;  // asked once, not on every call
        if (have < lds) {
            if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                (void)hipGetLastError();  // reported through the return code, not left pending
                refused = lds;
                return ATTN_ERR_LDS;
            }
            have = lds;
        }
    }
    void* args[] = {const_cast<AttnArgs*>(&a)};
    if (hipLaunchKernel(kern, grid, dim3(block), args, lds, st) == hipSuccess) return 0;
    (void)hipGetLastError();  // likewise
    return ATTN_ERR_LAUNCH;
}

int attn_cu_count() {
    static std::mutex mu;
    static std::map<int, int> cus;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    int& n = cus[dev];
    if (n <= 0 && (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)) n = 256;
    return n;
}

namespace {

// the partials of both kernels -> the slot's amax (state[1], zeroed by the roll): a grid-strided max, one
// atomic per block (a single block took 86 us for the 262 k partials of a GPT-2-medium step)
__global__ void __launch_bounds__(256) attn_amax_reduce_k(const float* __restrict__ part, int n, float* __restrict__ st) {
    __shared__ float red[4];
    float m = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) m = fmaxf(m, part[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicMax(reinterpret_cast<int*>(st + 1), __float_as_int(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// The MFMA kernels' requirements: D ∈ {32, 64, 128} and 16-B aligned rows (strides in elements).  The
// forward's form decides the units of lse (base 2 iff it holds); the backward needs it plus aligned
// gradient rows, so a backward that runs on MFMA always reads a base-2 lse.
bool mfma_head(int D) { return D == 32 || D == 64 || D == 128; }
bool fwd_aligned(const AttnArgs& a) {
    return mfma_head(a.D) && (a.q_st % 8 == 0) && (a.k_st % 8 == 0) && (a.v_st % 8 == 0) && (a.o_st % 4 == 0);
}
bool bwd_aligned(const AttnArgs& a) {
    return fwd_aligned(a) && (a.do_st % 8 == 0) && (a.o_st % 8 == 0) && (a.dq_st % 4 == 0) && (a.dk_st % 4 == 0) &&
           (a.dv_st % 4 == 0) && (a.o_sh % 8 == 0) && (a.do_sh % 8 == 0);
}

// What runs for a call: the family, the units of lse, and every workgroup count (the e5m2 amax partials
// are sized from the same dkdv_wgs the dK/dV kernel is launched with).
struct AttnPlan {
    AttnPath path;
    bool lse_log2;
    int groups;  // backward: 64-row groups per wave (dQ: 64·groups queries per workgroup, dK/dV: keys)
    unsigned fwd_wgs, dq_wgs, dkdv_wgs;
};

// Block order inside every grid: head-interleaved (blk_map).  An XCD-grouped order was measured slower
// (GPT-2-small causal B64: fwd 0.177 -> 0.199 ms, bwd 0.571 -> 0.597 ms: a head's 8 query blocks then read
// the same K/V tiles at the same moment) and was removed in round 4.
AttnPlan attn_select(const AttnArgs& a, bool backward, bool resident_ok = true) {
    const unsigned BH = a.B * a.H;
    auto blocks = [&](int T, int per) { return BH * (unsigned)((T + per - 1) / per); };
    const bool plain = !a.bias && a.p_drop == 0.f, small = a.Tq <= RES_T && a.Tk <= RES_T;
    AttnPlan p = {};
    p.lse_log2 = fwd_aligned(a);
    p.groups = 1;
    if (!(backward ? bwd_aligned(a) : p.lse_log2)) {
        p.path = AttnPath::Generic;  // (its grids are one workgroup per row: the launcher's)
    } else if (a.D != 64) {
        // D = 32 / 128: the bias / dropout capable single-loop forward (64 queries per workgroup at D = 128 to
        // fit the O accumulators), dQ (+ delta) then dK/dV with one 64-row group per wave
        p.path = AttnPath::Mfma;
        p.fwd_wgs = blocks(a.Tq, a.D == 128 ? 64 : 128);
    } else if (plain && small && resident_ok && (!backward || (!a.causal && !a.q8))) {
        // Tq, Tk <= 256 (ViT-B/16, T = 197): whole head resident.  Forward, one 8-wave workgroup per (b, h):
        // 0.205 -> 0.165 ms per layer (profiles/attention_resident_r6.txt).  Backward (non-causal, no e5m2
        // twin): persistent over the CUs, its grid is the launcher's.
        p.path = AttnPath::Resident;
        p.fwd_wgs = BH;
    } else if (plain && a.causal && !backward) {
        // the 32×32×16 forward with 8 waves (256 queries) per workgroup (GPT-2-small b64: 0.187 -> 0.179 ->
        // 0.170 ms per layer, profiles/attention_r6.txt, attention_memtraffic_r6.txt)
        p.path = AttnPath::Causal8;
        p.fwd_wgs = blocks(a.Tq, 256);
    } else if (plain) {
        // forward (non-causal): the 16×16×32 split-loop v2 kernel; backward (causal or not): two 64-query
        // groups per wave in dQ (bwd -11 % at GPT-2-small shapes) and two 64-key groups per wave in dK/dV
        // (-2.4 %, occupancy 2 at 240 VGPRs)
        p.path = AttnPath::Plain;
        p.groups = 2;
        p.fwd_wgs = blocks(a.Tq, 128);
    } else {
        // additive bias or dropout (the reference blocks): the single-loop forward, one group per wave
        p.path = AttnPath::BiasDrop;
        p.fwd_wgs = blocks(a.Tq, 128);
    }
    p.dq_wgs = blocks(a.Tq, 64 * p.groups);
    p.dkdv_wgs = blocks(a.Tk, 64 * p.groups);
    return p;
}

int launch_dq(const AttnArgs& a, const AttnPlan& p, hipStream_t st) {
    return a.D == 32 ? attn_launch_dq_d32(a, p.groups, p.dq_wgs, st)
         : a.D == 64 ? attn_launch_dq_d64(a, p.groups, p.dq_wgs, st)
                     : attn_launch_dq_d128(a, p.groups, p.dq_wgs, st);
}
int launch_dkdv(const AttnArgs& a, const AttnPlan& p, hipStream_t st) {
    return a.D == 32 ? attn_launch_dkdv_d32(a, p.groups, p.dkdv_wgs, st)
         : a.D == 64 ? attn_launch_dkdv_d64(a, p.groups, p.dkdv_wgs, st)
                     : attn_launch_dkdv_d128(a, p.groups, p.dkdv_wgs, st);
}

}  // namespace
}  // namespace rn_attn

using namespace rn_attn;

extern "C" {

int rn_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const float* bias, int bias_b,
                const long* strides, int B, int H, int Tq, int Tk, int D, float scale, int causal, float p_drop,
                uint64_t seed, const uint64_t* seed_ptr, hipStream_t st) {
    AttnArgs a = {};
    a.seed_ptr = seed_ptr;
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.o = (bf16*)o; a.lse = lse; a.bias = bias;
    a.q_sb = strides[0]; a.q_st = strides[1]; a.q_sh = strides[2];
    a.k_sb = strides[3]; a.k_st = strides[4]; a.k_sh = strides[5];
    a.v_sb = strides[6]; a.v_st = strides[7]; a.v_sh = strides[8];
    a.o_sb = strides[9]; a.o_st = strides[10]; a.o_sh = strides[11];
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.D = D; a.causal = causal; a.bias_b = bias_b;
    a.scale = scale; a.p_drop = p_drop; a.seed = seed;
    const AttnPlan plan = attn_select(a, false);
    switch (plan.path) {
    case AttnPath::Generic: return attn_launch_fwd_generic(a, st);
    case AttnPath::Resident:
    case AttnPath::Causal8: return attn_launch_fwd32(a, plan.path, plan.fwd_wgs, st);
    default: return attn_launch_fwd16(a, plan.path, plan.fwd_wgs, st);
    }
}

int rn_attn_bwd(const void* dout, const void* q, const void* k, const void* v, const void* o, const float* lse,
                const float* bias, int bias_b, void* dq, void* dk, void* dv, float* delta, const long* s, int B, int H,
                int Tq, int Tk, int D, float scale, int causal, float p_drop, uint64_t seed, const uint64_t* seed_ptr,
                float* bsum, void* q8, float* q8st, int q8_only, float* q8part, hipStream_t st) {
    AttnArgs a = {};
    // q8: the e5m2 twin of the buffer dq / dk / dv live in (same element offsets from dq)
    a.q8 = (uint8_t*)q8; a.q8st = q8st; a.q8_only = q8_only;
    if (q8) {
        a.q8k = (uint8_t*)q8 + ((const bf16*)dk - (const bf16*)dq);
        a.q8v = (uint8_t*)q8 + ((const bf16*)dv - (const bf16*)dq);
        // q8part: >= 8·B·H·ceil(T/64) floats (rn_attn_q8_part_floats): both kernels' per-wave partials
        a.q8part = q8part;
        a.q8part2 = q8part + 4L * B * H * ((Tq + 63) / 64);
    }
    a.seed_ptr = seed_ptr;
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.o = (bf16*)o; a.lse = (float*)lse;
    a.bias = bias; a.dout = (const bf16*)dout; a.dq = (bf16*)dq; a.dk = (bf16*)dk; a.dv = (bf16*)dv; a.delta = delta;
    a.q_sb = s[0]; a.q_st = s[1]; a.q_sh = s[2]; a.k_sb = s[3]; a.k_st = s[4]; a.k_sh = s[5];
    a.v_sb = s[6]; a.v_st = s[7]; a.v_sh = s[8]; a.o_sb = s[9]; a.o_st = s[10]; a.o_sh = s[11];
    a.do_sb = s[12]; a.do_st = s[13]; a.do_sh = s[14]; a.dq_sb = s[15]; a.dq_st = s[16]; a.dq_sh = s[17];
    a.dk_sb = s[18]; a.dk_st = s[19]; a.dk_sh = s[20]; a.dv_sb = s[21]; a.dv_st = s[22]; a.dv_sh = s[23];
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.D = D; a.causal = causal; a.bias_b = bias_b;
    a.scale = scale; a.p_drop = p_drop; a.seed = seed; a.bsum = bsum;
    AttnPlan plan = attn_select(a, true);
    a.lse_log2 = plan.lse_log2;
    const bool fast = plan.path != AttnPath::Generic;
    if (bsum && !(fast && Tq == Tk)) return -2;  // bias partials: fast self-attention path only
    if (q8 && !(fast && D == 64)) return -3;     // e5m2 dQKV: the D = 64 kernels only (the caller quantises instead)
    if (!fast) return attn_launch_bwd_generic(a, st);
    if (plan.path == AttnPath::Resident) {
        const int rc = attn_launch_bwd_resident(a, st);
        if (rc != ATTN_ERR_LDS) return rc;
        plan = attn_select(a, true, false);  // no 137 KiB of LDS on this device: the streaming pair
    }
    if (q8) {
        rn_fp8_roll_bf8(q8st, st);  // the consumer's delayed e5m2 scale, before both kernels
        if (hipMemsetAsync(q8part, 0, (size_t)rn_attn_q8_part_floats(B, H, Tq, Tk) * sizeof(float), st) != hipSuccess)
            return ATTN_ERR_LAUNCH;
    }
    // dQ first: it also produces delta = rowsum(dO∘O), which the dK/dV kernel reads
    if (const int rc = launch_dq(a, plan, st)) return rc;
    if (const int rc = launch_dkdv(a, plan, st)) return rc;
    if (q8) {  // (the buffer was zeroed before the launches: a wave that never reaches its store leaves 0)
        int n = (int)(a.q8part2 - a.q8part) + 4 * (int)plan.dkdv_wgs;
        void* args[] = {&a.q8part, &n, &q8st};
        if (hipLaunchKernel((const void*)attn_amax_reduce_k, dim3(std::min(256, (n + 4095) / 4096)), dim3(256), args, 0,
                            st) != hipSuccess) {
            (void)hipGetLastError();
            return ATTN_ERR_LAUNCH;
        }
    }
    return 0;
}

int rn_attn_is_fast(int D) { return mfma_head(D); }
long rn_attn_q8_part_floats(int B, int H, int Tq, int Tk) {
    return 4L * B * H * ((Tq + 63) / 64) + 4L * B * H * ((Tk + 63) / 64);
}

}  // extern "C"
