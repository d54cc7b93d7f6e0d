// Speculative sampling: verification of K draft tokens per batch row, on the device, two launches.
//
// verify_k    one workgroup of 1024 threads per (row b, window position i), B · (K + 1) of them.  It
//             reads its target row once as 16-byte vectors into registers (as in sampling.hip: the
//             order-preserving keys, 7 rounds of one vector) and, for i < K, its draft row the same
//             way, finds each row's maximum, top-k / top-p threshold and Z with the one-bit radix
//             select and fixed-tree reductions of sampling_common.h, and decides position i:
//               accepted     u_acc · q(d) < p(d) with q(d) > 0, d = drafts[b, i]   (i < K)
//               candidate    the token the row commits if i is its first rejected position: a draw
//                            from the residual max(p - q, 0), from p where that has no mass, and
//                            for i = K the bonus token drawn from p.  An accepted position's
//                            candidate is never read and is not drawn.
//             Both go to one int32 per position: bit 31 = accepted, the rest the candidate.
// combine_k   one thread per row: the number a of leading accepted positions, then
//             tokens[b] = d_1 .. d_a, candidate[a], 0 ...; matched[b] = a.
//
// Registers: at 1024 threads a wave has 128 VGPRs; sample_k's 28 key + 56 mass registers per bf16
// row do not fit twice.  Both rows' KEYS are held (2 × 28) and a pass that needs masses recomputes
// them with v_exp_f32 (Row<.., E = false>): the residual needs p and q of the same index side by
// side, and the passes are few (the select's, then four over the rows for the draw).  The draft row
// is read in the TARGET row's slot mapping, so that a thread holds both rows' values of the same
// indices; where the two row starts sit differently against a 16-byte boundary the draft row is
// read element by element (decoding pads its draft buffer's rows so that this never happens).
// Rows longer than 7 rounds re-read both rows from memory in every pass (R = 0): correct only.
//
// temperature == 0: p is one-hot at the target's argmax (lowest index on ties): accepted iff d is
// that argmax, the candidate is the argmax; the draft row is not read.
//
// Determinism as in sampling.hip: no atomics, no cross-workgroup wait, fixed trees.
#include "rn_api.h"
#include "sampling_common.h"

namespace {

constexpr uint32_t SV_ACCEPTED = 0x80000000u;

// max(p - q, 0) of the normalised masses.  No contraction: an fma would turn equal products (the
// draft row equal to the target row) into their rounding error instead of 0.
RN_DEV float residual(float ep, float rzp, float eq, float rzq) {
#pragma clang fp contract(off)
    const float p = ep * rzp, q = eq * rzq;
    return p > q ? p - q : 0.f;
}

// f(index, kp, ep, kq, eq) for the slots of round jsel of both rows (one slot mapping), in index order
template <typename T, int R, class F>
RN_DEV void visit_both(const Row<T, R, false>& p, const Row<T, R, false>& q, int jsel, F&& f) {
    constexpr int VEC = Row<T, R, false>::VEC;
    if constexpr (R > 0) {
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (j == jsel) {
                const uint32_t z = Row<T, R, false>::salt();
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const uint32_t kp = p.key(j * VEC + v, z), kq = q.key(j * VEC + v, z);
                    f(p.index(j, v, z), kp, p.mass(kp), kq, q.mass(kq));
                }
            }
    } else {
        uint32_t kp[VEC], kq[VEC];
        p.load_round(jsel, kp);
        q.load_round(jsel, kq);
#pragma unroll
        for (int v = 0; v < VEC; ++v) f(p.index(jsel, v), kp[v], p.mass(kp[v]), kq[v], q.mass(kq[v]));
    }
}

template <typename T, int R>
__global__ void __launch_bounds__(SMP_T) verify_k(const T* __restrict__ tl, long tld_b, long tld_i,
                                                  const T* __restrict__ dl, long dld_b, long dld_i,
                                                  const int64_t* __restrict__ drafts, int K, int V, float temperature,
                                                  int top_k, float top_p, const float* __restrict__ params,
                                                  const float* __restrict__ u_in, const uint64_t* __restrict__ seed,
                                                  uint32_t* __restrict__ cand) {
    using RowT = Row<T, R, false>;
    __shared__ unsigned long long red[2][SMP_W];
    __shared__ float wave_tot[SMP_W];
    Reducer reduce{red};
    const int w = blockIdx.x, b = w / (K + 1), i = w - b * (K + 1), tid = threadIdx.x;

    RowT rp;
    const T* prow = tl + (long)b * tld_b + (long)i * tld_i;
    rp.open(prow, V, RowT::start(prow));
    smp_settings(params, temperature, top_k, top_p);

    int d = -1;  // the draft token; outside [0, V) (the binding's check may be off): rejected, never an index
    if (i < K) {
        const int64_t d64 = drafts[(long)b * K + i];
        d = d64 >= 0 && d64 < V ? (int)d64 : -1;
    }
    uint32_t Mp, bkp;
    const int amax = smp_argmax(rp, reduce, Mp, bkp);
    if (!(temperature > 0.f)) {  // greedy
        if (tid == 0) cand[w] = (uint32_t)amax | (d == amax ? SV_ACCEPTED : 0u);
        return;
    }
    const float c2 = 1.4426950408889634f / temperature;
    rp.m = key2f<T>(Mp);
    rp.c2 = c2;
    const uint32_t thrp = smp_threshold<T>(rp, reduce, Mp, bkp, top_k, top_p);
    const auto p_mass = [&](int j, auto&& f) {
        rp.visit_round(j, [&](int n, uint32_t k, float e) { f(n, k >= thrp ? e : 0.f); });
    };
    float ua, ud;
    if (u_in) {
        ua = u_in[2 * (long)w];
        ud = u_in[2 * (long)w + 1];
    } else {
        ua = hash_uniform(*seed, 2 * (uint64_t)w);
        ud = hash_uniform(*seed, 2 * (uint64_t)w + 1);
    }

    int tok = -1, owner = SMP_NONE;
    if (i < K) {
        RowT rq;
        const T* qrow = dl + (long)b * dld_b + (long)i * dld_i;
        rq.open(qrow, V, rp.off);  // the target row's slots
        uint32_t Mq, bkq;
        smp_argmax(rq, reduce, Mq, bkq);
        rq.m = key2f<T>(Mq);
        rq.c2 = c2;
        const uint32_t thrq = smp_threshold<T>(rq, reduce, Mq, bkq, top_k, top_p);
        const auto q_mass = [&](int j, auto&& f) {
            rq.visit_round(j, [&](int n, uint32_t k, float e) { f(n, k >= thrq ? e : 0.f); });
        };
        // every row holds its maximum, of mass 1: Z >= 1
        const float Zp = smp_total(p_mass, rp.rounds, reduce), Zq = smp_total(q_mass, rp.rounds, reduce);
        if (d >= 0) {  // p(d), q(d): every thread reads the two logits (one broadcast load each)
            const uint32_t kp = f2key<T>((float)prow[d]), kq = f2key<T>((float)qrow[d]);
            const float pd = (kp >= thrp ? rp.mass(kp) : 0.f) / Zp, qd = (kq >= thrq ? rq.mass(kq) : 0.f) / Zq;
            ua = ua >= 0.f ? (ua < 1.f ? ua : 0.99999994f) : 0.f;
            if (qd > 0.f && ua * qd < pd) {  // block-uniform
                if (tid == 0) cand[w] = SV_ACCEPTED;
                return;
            }
        }
        const float rzp = 1.f / Zp, rzq = 1.f / Zq;
        const auto res_mass = [&](int j, auto&& f) {
            visit_both<T, R>(rp, rq, j, [&](int n, uint32_t kp, float ep, uint32_t kq, float eq) {
                f(n, residual(kp >= thrp ? ep : 0.f, rzp, kq >= thrq ? eq : 0.f, rzq));
            });
        };
        owner = smp_draw(res_mass, rp.rounds, ud, reduce, wave_tot, tok);
    }
    if (owner == SMP_NONE)  // the bonus position, or a residual without mass: from p (Z >= 1: never without)
        owner = smp_draw(p_mass, rp.rounds, ud, reduce, wave_tot, tok);
    if (owner == SMP_NONE ? tid == 0 : tid == owner)
        cand[w] = (uint32_t)(owner == SMP_NONE || tok < 0 || tok >= V ? amax : tok);
}

__global__ void combine_k(const uint32_t* __restrict__ cand, const int64_t* __restrict__ drafts, int B, int K,
                          int64_t* __restrict__ tokens, int64_t* __restrict__ matched) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t* c = cand + (long)b * (K + 1);
    int a = 0;
    while (a < K && (c[a] & SV_ACCEPTED)) ++a;
    for (int i = 0; i <= K; ++i)
        tokens[(long)b * (K + 1) + i] = i < a ? drafts[(long)b * K + i] : i == a ? (int64_t)(c[a] & ~SV_ACCEPTED) : 0;
    matched[b] = a;
}

template <typename T>
int launch(const void* tl, const long* tld, const void* dl, const long* dld, const int64_t* drafts, int B, int K, int V,
           float temperature, int top_k, float top_p, const float* params, const float* u, const uint64_t* seed,
           uint32_t* cand, int64_t* tokens, int64_t* matched, hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T), PER = SMP_T * VEC;  // slots per round
    constexpr int RFULL = 7;                                     // 28 packed bf16 key registers per row
    const long slots = (long)V + VEC - 1;                        // the row start may sit VEC - 1 into a vector
#define RN_VERIFY(R_)                                                                                              \
    verify_k<T, R_><<<B*(K + 1), SMP_T, 0, st>>>((const T*)tl, tld[0], tld[1], (const T*)dl, dld[0], dld[1], drafts, K, \
                                                   V, temperature, top_k, top_p, params, u, seed, cand)
    if (slots <= PER) RN_VERIFY(1);
    else if (slots <= (long)RFULL * PER) RN_VERIFY(RFULL);
    else RN_VERIFY(0);
#undef RN_VERIFY
    HIP_CHECK_LAUNCH();
    combine_k<<<(B + 255) / 256, 256, 0, st>>>(cand, drafts, B, K, tokens, matched);
    HIP_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int rn_spec_verify(const void* target, const long* tld, const void* draft, const long* dld,
                              const int64_t* drafts, int is_bf16, int B, int K, int V, float temperature, int top_k,
                              float top_p, const float* params, const float* u, const uint64_t* seed, uint32_t* cand,
                              int64_t* tokens, int64_t* matched, hipStream_t st) {
    if (B < 1 || K < 1 || K > 15 || V < 1 || V > (1 << 30) || (long)B * (K + 1) > (1 << 30) || tld[1] < V || dld[1] < V ||
        (u == nullptr) == (seed == nullptr))
        return 1;
    return is_bf16 ? launch<bf16>(target, tld, draft, dld, drafts, B, K, V, temperature, top_k, top_p, params, u, seed,
                                  cand, tokens, matched, st)
                   : launch<float>(target, tld, draft, dld, drafts, B, K, V, temperature, top_k, top_p, params, u, seed,
                                   cand, tokens, matched, st);
}
