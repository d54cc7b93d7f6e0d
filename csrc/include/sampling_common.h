// What the token sampler (sampling.hip) and the speculative verifier (spec_verify.hip) share: a
// 1024-thread workgroup's view of one row of logits as order-preserving integer keys, the fixed-tree
// block reduce, and — as functions, for the verifier — the one-bit radix selects of the top-k /
// top-p threshold and the three-level inverse-CDF draw over any weights (sample_k keeps the same
// loops written out: see the note in sampling.hip).  See sampling.hip for the method; everything
// here is deterministic (integer counts, fixed float trees, no atomics).
#pragma once

#include "common.h"

namespace {  // internal linkage: every TU gets its own copy

constexpr int SMP_T = 1024, SMP_W = SMP_T / RN_WAVE;

// order-preserving image of a float: a > b  <=>  key(a) > key(b); NaN counts as -inf, -0 as +0.
// Every valid key is >= key(-inf) = 0x007fffff, so 0 marks a slot outside the row.
// A bf16 key keeps its 16 significant bits on top and zeros below (two of them share a register).
template <typename T>
RN_DEV uint32_t f2key(float x) {
    if (x != x) x = -INFINITY;
    x += 0.f;
    const uint32_t b = __float_as_uint(x);
    const uint32_t k = b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return sizeof(T) == 2 ? k & 0xFFFF0000u : k;
}
template <typename T>
RN_DEV float key2f(uint32_t k) {
    const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    return __uint_as_float(sizeof(T) == 2 ? b & 0xFFFF0000u : b);
}

RN_DEV void ldvec(const bf16* p, float* f) { load8(p, f); }
RN_DEV void ldvec(const float* p, float* f) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = v[i];
}

// A thread's view of its row.  Slot s = (round · 1024 + thread) · VEC + q holds row index s - off,
// where off (< VEC) is how far the row start lies past a 16-byte boundary: vectors that lie inside
// the row are aligned whatever the row stride; the head and tail vectors are read element by element.
// (A row read in ANOTHER row's slot mapping — the verifier's draft row — has vec = false unless the
// two starts sit equally far past a boundary: then every slot is read element by element.)
// R rounds are kept in registers as keys (R = 0: every pass re-reads the row from memory); with E
// their masses are kept too (fill_masses), without it a pass that needs a mass recomputes the exp2.
template <typename T, int R, bool E = true>
struct Row {
    static constexpr int VEC = 16 / (int)sizeof(T), N = R > 0 ? R * VEC : 1;
    static constexpr bool PACK = sizeof(T) == 2;  // two 16-bit keys per register
    const T* row;
    int V, off, rounds;
    bool vec;
    float m, c2;  // e = exp2((x - m) · c2)
    uint32_t keys[PACK ? (N + 1) / 2 : N];
    float e[E ? N : 1];

    // the view of `p` in the slot mapping of offset `o` (its own: o = start(p)), keys loaded
    RN_DEV static int start(const T* p) { return (int)((reinterpret_cast<uintptr_t>(p) / sizeof(T)) % VEC); }
    RN_DEV void open(const T* p, int V_, int o) {
        row = p;
        V = V_;
        off = o;
        vec = start(p) == o;
        rounds = (V + off + SMP_T * VEC - 1) / (SMP_T * VEC);
        m = 0.f;
        c2 = 0.f;
        if constexpr (R > 0) {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                uint32_t k[VEC];
                load_round(j, k);
                set_keys(j, k);
            }
        }
    }
    RN_DEV void fill_masses() {
        if constexpr (R > 0 && E) {
#pragma unroll
            for (int n = 0; n < R * VEC; ++n) e[n] = mass(key(n));
        }
    }

    // A pass's salt: 0, but without kept masses opaque to the compiler, which would otherwise hoist the
    // unpacked keys and their exp2 out of the selects' bit loops and keep every slot's index live from
    // one pass to the next — the very register footprint that E = false is there to avoid.
    RN_DEV static uint32_t salt() {
        uint32_t z = 0;
        if constexpr (!E) asm volatile("" : "+s"(z));
        return z;
    }
    RN_DEV uint32_t key(int n, uint32_t z = 0) const {
        if constexpr (PACK) return (n & 1) ? (keys[n / 2] | z) & 0xFFFF0000u : (keys[n / 2] | z) << 16;
        else return keys[n] | z;
    }
    RN_DEV void set_keys(int j, const uint32_t* k) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            if constexpr (!PACK) keys[j * VEC + q] = k[q];
            else if (q & 1) keys[(j * VEC + q) / 2] = k[q] | (k[q - 1] >> 16);
        }
    }

    RN_DEV int index(int j, int q, uint32_t z = 0) const { return (j * SMP_T + (int)threadIdx.x) * VEC + q - off - (int)z; }
    RN_DEV float mass(uint32_t k) const {
        if constexpr (E) {  // computed once per slot (fill_masses)
            if (k == 0) return 0.f;
            const float x = key2f<T>(k);
            return x == m ? 1.f : __builtin_amdgcn_exp2f((x - m) * c2);
        } else {  // in every pass: straight-line (selects, no early return), or 56 slots become 56 branches
            const float x = key2f<T>(k);
            const float e = __builtin_amdgcn_exp2f((x - m) * c2);
            return k == 0 ? 0.f : (x == m ? 1.f : e);
        }
    }
    RN_DEV void load_round(int j, uint32_t* k) const {
        const int i0 = index(j, 0);
        if (vec && i0 >= 0 && i0 <= V - VEC) {
            float f[VEC];
            ldvec(row + i0, f);
#pragma unroll
            for (int q = 0; q < VEC; ++q) k[q] = f2key<T>(f[q]);
        } else {
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const int i = i0 + q;
                k[q] = 0u;
                if (i >= 0 && i < V) k[q] = f2key<T>((float)row[i]);
            }
        }
    }
    template <class F>
    RN_DEV void slot(int j, int q, uint32_t z, F&& f) const {  // a register slot: its key, its mass kept or recomputed
        const uint32_t k = key(j * VEC + q, z);
        if constexpr (E) f(index(j, q), k, e[j * VEC + q]);
        else f(index(j, q, z), k, mass(k));
    }
    // f(index, key, e) for the slots of round jsel / of every round, in index order
    template <class F>
    RN_DEV void visit_round(int jsel, F&& f) const {
        if constexpr (R > 0) {
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (j == jsel) {  // (the salt in here also keeps this chain from becoming an indexed, memory-held array)
                    const uint32_t z = salt();
#pragma unroll
                    for (int q = 0; q < VEC; ++q) slot(j, q, z, f);
                }
        } else {
            uint32_t k[VEC];
            load_round(jsel, k);
#pragma unroll
            for (int q = 0; q < VEC; ++q) f(index(jsel, q), k[q], mass(k[q]));
        }
    }
    template <class F>
    RN_DEV void visit(F&& f) const {
        if constexpr (R > 0) {
            const uint32_t z = salt();
#pragma unroll
            for (int j = 0; j < R; ++j) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) slot(j, q, z, f);
                // recomputed masses: one vector's worth of temporaries at a time, not the whole row's
                if constexpr (!E) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            for (int j = 0; j < rounds; ++j) visit_round(j, f);
        }
    }
};

// Block-wide reduce, the result in every thread: xor butterfly, then the 16 wave partials in order
// (a fixed tree).  Two LDS buffers used in turn, so one barrier per reduce is enough: a wave can
// only write a buffer again after every wave has passed the barrier of the reduce in between.
struct Reducer {
    unsigned long long (*buf)[SMP_W];
    int par = 0;
    template <typename V, class Op>
    RN_DEV V operator()(V v, Op op) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
        V* s = reinterpret_cast<V*>(buf[par]);
        par ^= 1;
        if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
        __syncthreads();
        V t = s[0];
#pragma unroll
        for (int i = 1; i < SMP_W; ++i) t = op(t, s[i]);
        return t;
    }
};

RN_DEV auto smp_add() { return [](auto a, auto b) { return a + b; }; }
RN_DEV auto smp_max() { return [](auto a, auto b) { return a > b ? a : b; }; }
RN_DEV auto smp_min() { return [](auto a, auto b) { return a < b ? a : b; }; }

// device settings override the host ones: one captured graph serves every setting
RN_DEV void smp_settings(const float* params, float& temperature, int& top_k, float& top_p) {
    if (params) {
        temperature = params[0];
        const float kf = params[1];
        top_k = kf >= 1.f && kf < 1073741824.f ? (int)kf : 0;
        top_p = params[2];
    }
}

// The row's largest key M and its index, lowest on ties (the thread visits its slots in index
// order); bk: this thread's own largest key.
template <class RowT>
RN_DEV int smp_argmax(const RowT& r, Reducer& reduce, uint32_t& M, uint32_t& bk) {
    bk = 0;
    int bi = 0;
    r.visit([&](int i, uint32_t k, float) {
        if (k > bk) {
            bk = k;
            bi = i;
        }
    });
    const unsigned long long best = reduce(((unsigned long long)bk << 32) | (uint32_t)~bi, smp_max());
    M = (uint32_t)(best >> 32);
    const int amax = (int)~(uint32_t)best;
    return amax < 0 ? 0 : (amax >= r.V ? r.V - 1 : amax);
}

// The kept set of the filters as a key threshold: a token is kept iff key >= the result (<= M).
// r.m / r.c2 (and the masses of a Row that keeps them) are set; M, bk: from smp_argmax.
template <typename T, class RowT>
RN_DEV uint32_t smp_threshold(const RowT& r, Reducer& reduce, uint32_t M, uint32_t bk, int top_k, float top_p) {
    constexpr int LOW_BIT = 32 - 8 * (int)sizeof(T);  // bf16 keys: the low 16 bits carry no order
    const auto add = smp_add();
    // top-k: thr = the k-th largest key = the largest t with #{key >= t} >= k, one bit at a time
    uint32_t thr = 0;
    if (top_k >= 1 && top_k < r.V) {
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
    return thr < M ? thr : M;
}

// Σ of the weights: per-round block sums added in round order.  weights(j, f) calls f(index, w) for
// this thread's slots of round j in index order.
template <class W>
RN_DEV float smp_total(W&& weights, int rounds, Reducer& reduce) {
    float Z = 0.f;
    for (int j = 0; j < rounds; ++j) {
        float w = 0.f;
        weights(j, [&](int, float x) { w += x; });
        Z += reduce(w, smp_add());
    }
    return Z;
}

// Inverse-CDF draw in index order over non-negative weights, three levels: round totals -> one block
// scan inside the hit round -> the owning thread's vector.  A level picks the first unit with
// cumulative weight > u·Z AND weight > 0, else its last unit with weight > 0, so the index returned
// always has a non-zero weight.  Block-uniform result: SMP_NONE when no weight is positive, else the
// number of the one thread that holds the drawn index in `tok` (-1 there: none found, not reachable).
constexpr int SMP_NONE = -1;
template <class W>
RN_DEV int smp_draw(W&& weights, int rounds, float u, Reducer& reduce, float* wave_tot, int& tok) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const auto round_sum = [&](int j) {
        float w = 0.f;
        weights(j, [&](int, float x) { w += x; });
        return reduce(w, smp_add());
    };
    // level 1: per-round weights, Z their sum in round order
    float Z = 0.f;
    for (int j = 0; j < rounds; ++j) Z += round_sum(j);
    u = u >= 0.f ? (u < 1.f ? u : 0.99999994f) : 0.f;
    float target = u * Z;
    int jsel = -1, jlast = -1;
    float Psel = 0.f, Plast = 0.f, P = 0.f;
    for (int j = 0; j < rounds; ++j) {
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
    if (jlast < 0) return SMP_NONE;
    if (jsel < 0) {  // rounding left none: the last index of non-zero weight
        jsel = jlast;
        Psel = Plast;
        target = INFINITY;
    }

    // level 2: inclusive scan of the threads' weights inside the hit round
    float w = 0.f;
    weights(jsel, [&](int, float x) { w += x; });
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
    int tsel = reduce(hit, smp_min());
    const int tlast = reduce(w > 0.f ? tid : -1, smp_max());
    if (tsel == SMP_T) {
        tsel = tlast;
        target = INFINITY;
    }

    // level 3: the owning thread walks its vector
    if (tid == tsel) {
        float c = base + excl;
        int last = -1;
        tok = -1;
        weights(jsel, [&](int i, float x) {
            if (x > 0.f) {
                c += x;
                last = i;
                if (tok < 0 && c > target) tok = i;
            }
        });
        if (tok < 0) tok = last;
    }
    return tsel;
}

}  // namespace
