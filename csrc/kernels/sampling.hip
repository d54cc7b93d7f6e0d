// Fused token sampler: temperature, top-k, top-p (nucleus) and the draw, one launch per decode step.
//
// One workgroup of 1024 threads per row of logits (B, V).  Each thread reads its share of the row
// ONCE, as 16-byte vectors, into registers (R rounds of one vector: 56 values per thread at
// V = 50257) as order-preserving integer keys, and everything below runs from those registers:
//
//   max / argmax   one block reduce of (key, ~index): the largest key, lowest index on ties
//   top-k          the k-th largest key by radix select with ONE-BIT digits: for every key bit from
//                  the top, count the keys >= prefix | bit (block reduce of integers) and keep the
//                  bit when at least k are.  At most 16 counts for bf16, 32 for fp32, and a pass
//                  over the row only for the bits on which the maximum and a lower bound (the
//                  k-th largest of the 1024 thread maxima, found the same way from one key per
//                  thread) differ.  No LDS histogram: bf16 logits cluster in a handful of 8-bit
//                  digits, where LDS atomics serialise.
//   top-p          the same select weighted by e = exp((x - max) / T): the largest threshold t whose
//                  mass of keys >= t still reaches top_p · Z (passes only between the top-k
//                  threshold and the maximum).  Exactly "keep a token iff the mass of
//                  the strictly greater logits is < top_p": whole tie groups stay or go.
//   draw           inverse CDF in vocabulary index order, three levels: round totals -> one block
//                  scan inside the hit round -> the owning thread's vector.
//
// Determinism: counts are integers, every float sum is a fixed tree (thread order, xor butterfly,
// 16 wave partials in order) — no atomics at all, so equal inputs give equal outputs bitwise.
// The draw is robust to the different association of its levels: a level picks the first unit with
// cumulative mass > u·Z AND mass > 0, else its last unit with mass > 0, so the token returned is
// always a kept one of non-zero probability (never a -inf logit), at most a rounding away from the
// exact inverse CDF.
//
// Rows longer than the register budget (V + 7 > 57344) re-read the row from global memory in every
// pass (R = 0): that path only has to be correct.
//
// Row, Reducer and the key maps live in sampling_common.h, shared with spec_verify.hip.  The select
// loops and the draw stay written out here although the header has them as functions (smp_threshold,
// smp_draw) for the verifier: behind those calls this kernel's register allocation changed (336
// instead of 296 bytes of spills for bf16 rows) and the sampled decode step at batch 64 took 0.10
// instead of 0.07 ms more than the greedy one.
#include "rn_api.h"
#include "sampling_common.h"

namespace {

template <typename T, int R>
__global__ void __launch_bounds__(SMP_T) sample_k(const T* __restrict__ logits, long ld, int V, float temperature,
                                                  int top_k, float top_p, const float* __restrict__ params,
                                                  const float* __restrict__ u_in, const uint64_t* __restrict__ seed,
                                                  int64_t* __restrict__ tokens, int* __restrict__ kept) {
    constexpr int VEC = Row<T, R>::VEC;
    constexpr int LOW_BIT = 32 - 8 * (int)sizeof(T);  // bf16 keys: the low 16 bits carry no order
    __shared__ unsigned long long red[2][SMP_W];
    __shared__ float wave_tot[SMP_W];
    Reducer reduce{red};
    const auto add = [](auto a, auto b) { return a + b; };
    const auto mx = [](auto a, auto b) { return a > b ? a : b; };
    const auto mn = [](auto a, auto b) { return a < b ? a : b; };
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    Row<T, R> r;
    r.row = logits + (long)b * ld;
    r.V = V;
    r.vec = true;  // the row in its own slot mapping: aligned vectors
    r.off = (int)((reinterpret_cast<uintptr_t>(r.row) / sizeof(T)) % VEC);
    r.rounds = (V + r.off + SMP_T * VEC - 1) / (SMP_T * VEC);
    r.m = 0.f;
    r.c2 = 0.f;
    if constexpr (R > 0) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            uint32_t k[VEC];
            r.load_round(j, k);
            r.set_keys(j, k);
        }
    }
    if (params) {  // device settings override the host ones: one captured graph serves every setting
        temperature = params[0];
        const float kf = params[1];
        top_k = kf >= 1.f && kf < 1073741824.f ? (int)kf : 0;
        top_p = params[2];
    }

    // largest key, lowest index on ties (the thread visits its slots in index order)
    uint32_t bk = 0;
    int bi = 0;
    r.visit([&](int i, uint32_t k, float) {
        if (k > bk) {
            bk = k;
            bi = i;
        }
    });
    const unsigned long long best = reduce(((unsigned long long)bk << 32) | (uint32_t)~bi, mx);
    const uint32_t M = (uint32_t)(best >> 32);
    int amax = (int)~(uint32_t)best;
    amax = amax < 0 ? 0 : (amax >= V ? V - 1 : amax);
    if (!(temperature > 0.f)) {  // greedy
        if (tid == 0) {
            tokens[b] = amax;
            kept[b] = 1;
        }
        return;
    }

    // the masses first: the floats just loaded are still in registers
    r.m = key2f<T>(M);
    r.c2 = 1.4426950408889634f / temperature;
    if constexpr (R > 0) {
#pragma unroll
        for (int n = 0; n < R * VEC; ++n) r.e[n] = r.mass(r.key(n));
    }

    // top-k: thr = the k-th largest key = the largest t with #{key >= t} >= k, one bit at a time
    uint32_t thr = 0;
    if (top_k >= 1 && top_k < V) {
        // a lower bound first, from one key per thread: k thread maxima >= c are k keys >= c
        uint32_t low = 0;
        for (int bit = 31; bit >= LOW_BIT; --bit) {
            const uint32_t c = low | (1u << bit);
            if (c <= M && reduce((int)(bk >= c), add) >= top_k) low = c;
        }
        for (int bit = 31; bit >= LOW_BIT; --bit) {
            const uint32_t c = thr | (1u << bit);
            if (c > M) continue;  // nothing is that large
            if (c <= low) {       // at least k are: no pass over the row
                thr = c;
                continue;
            }
            int n = 0;
            r.visit([&](int, uint32_t k, float) { n += k >= c; });
            if (reduce(n, add) >= top_k) thr = c;
        }
    }

    // top-p over the top-k set: the largest t whose mass of keys >= t reaches top_p · Z; a key >= t
    // then has less than top_p of the mass strictly above it.  The largest key always stays.
    if (top_p < 1.f) {
        float z = 0.f;
        r.visit([&](int, uint32_t k, float e) { z += k >= thr ? e : 0.f; });
        const float need = top_p * reduce(z, add);
        uint32_t t = M;
        if (need > 0.f) {
            t = 0;
            for (int bit = 31; bit >= LOW_BIT; --bit) {
                const uint32_t c = t | (1u << bit);
                if (c > M) continue;
                if (c <= thr) {  // the whole top-k set: its mass is Z
                    t = c;
                    continue;
                }
                const uint32_t cc = c;
                    float q = 0.f;
                r.visit([&](int, uint32_t k, float e) { q += k >= cc ? e : 0.f; });
                if (reduce(q, add) >= need) t = c;
            }
        }
        thr = t > thr ? t : thr;
    }
    thr = thr < M ? thr : M;

    // level 1: per-round masses of the kept set, Z their sum in round order
    int cnt = 0;
    r.visit([&](int, uint32_t k, float) { cnt += k != 0 && k >= thr; });
    cnt = reduce(cnt, add);
    const auto round_sum = [&](int j) {
        float w = 0.f;
        r.visit_round(j, [&](int, uint32_t k, float e) { w += k >= thr ? e : 0.f; });
        return reduce(w, add);
    };
    float Z = 0.f;
    for (int j = 0; j < r.rounds; ++j) Z += round_sum(j);
    float u = u_in ? u_in[b] : hash_uniform(*seed, (uint64_t)b);
    u = u >= 0.f ? (u < 1.f ? u : 0.99999994f) : 0.f;
    float target = u * Z;
    int jsel = -1, jlast = -1;
    float Psel = 0.f, Plast = 0.f, P = 0.f;
    for (int j = 0; j < r.rounds; ++j) {
        const float S = round_sum(j);  // the same tree as above: the same value
        if (S > 0.f) {
            jlast = j;
            Plast = P;
            if (jsel < 0 && P + S > target) {
                jsel = j;
                Psel = P;
            }
        }
        P += S;
    }
    if (jlast < 0) {  // no mass at all (not reachable for finite settings): the argmax
        if (tid == 0) {
            tokens[b] = amax;
            kept[b] = cnt;
        }
        return;
    }
    if (jsel < 0) {  // rounding left none: the last kept token of non-zero mass
        jsel = jlast;
        Psel = Plast;
        target = INFINITY;
    }

    // level 2: inclusive scan of the threads' masses inside the hit round
    float w = 0.f;
    r.visit_round(jsel, [&](int, uint32_t k, float e) { w += k >= thr ? e : 0.f; });
    float incl = w;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    float base = Psel;
    for (int i = 0; i < wid; ++i) base += wave_tot[i];
    const int hit = w > 0.f && base + incl > target ? tid : SMP_T;
    int tsel = reduce(hit, mn);
    const int tlast = reduce(w > 0.f ? tid : -1, mx);
    if (tsel == SMP_T) {
        tsel = tlast;
        target = INFINITY;
    }

    // level 3: the owning thread walks its vector
    if (tid == tsel) {
        float c = base + excl;
        int tok = -1, last = -1;
        r.visit_round(jsel, [&](int i, uint32_t k, float e) {
            if (k >= thr && e > 0.f) {
                c += e;
                last = i;
                if (tok < 0 && c > target) tok = i;
            }
        });
        if (tok < 0) tok = last;
        if (tok < 0 || tok >= V) tok = amax;
        tokens[b] = tok;
        kept[b] = cnt;
    }
}

template <typename T>
int launch(const void* logits, long ld, int B, int V, float temperature, int top_k, float top_p, const float* params,
           const float* u, const uint64_t* seed, int64_t* tokens, int* kept, hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T), PER = SMP_T * VEC;  // slots per round
    constexpr int RFULL = 56 / VEC;                              // 56 values per thread in registers
    const long slots = (long)V + VEC - 1;                        // the row start may sit VEC - 1 into a vector
#define RN_SAMPLE(R_) \
    sample_k<T, R_><<<B, SMP_T, 0, st>>>((const T*)logits, ld, V, temperature, top_k, top_p, params, u, seed, tokens, kept)
    if (slots <= PER) RN_SAMPLE(1);
    else if (slots <= (long)RFULL * PER) RN_SAMPLE(RFULL);
    else RN_SAMPLE(0);
#undef RN_SAMPLE
    HIP_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int rn_sample_logits(const void* logits, int is_bf16, long ld, int B, int V, float temperature, int top_k,
                                float top_p, const float* params, const float* u, const uint64_t* seed,
                                int64_t* tokens, int* kept, hipStream_t st) {
    if (B < 1 || V < 1 || V > (1 << 30) || ld < V || (u == nullptr) == (seed == nullptr)) return 1;
    return is_bf16 ? launch<bf16>(logits, ld, B, V, temperature, top_k, top_p, params, u, seed, tokens, kept, st)
                   : launch<float>(logits, ld, B, V, temperature, top_k, top_p, params, u, seed, tokens, kept, st);
}
