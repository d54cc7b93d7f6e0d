// Attention for head sizes without an MFMA kernel (any D <= 256) or unaligned rows: per-query-row kernels
// with fp32 scores in LDS; the backward is dQ (+ delta) per query row, then dK/dV per key row — no atomics,
// bitwise repeatable.  lse is the natural log here (AttnArgs::lse_log2 tells the backward which it got).
#include "attention_common.h"

namespace rn_attn {
namespace {

constexpr float LN2 = 0.6931471805599453f;

RN_DEV float bias_at(const AttnArgs& p, int b, int qi, int kj) {
    return p.bias ? p.bias[((long)(p.bias_b > 1 ? b : 0) * p.Tq + qi) * p.Tk + kj] : 0.f;
}
RN_DEV bool visible(const AttnArgs& p, int qi, int kj) { return !(p.causal && kj > qi + (p.Tk - p.Tq)); }

// one block per (b, h, q); scores in LDS (Tk floats)
__global__ void __launch_bounds__(256) attn_fwd_generic_k(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);
    float* qv = sc + p.Tk;
    __shared__ float red[16];
    const int qi = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const bf16* qp = p.q + b * p.q_sb + (long)qi * p.q_st + h * p.q_sh;
    for (int d = threadIdx.x; d < p.D; d += 256) qv[d] = bf2f(qp[d]);
    __syncthreads();
    float mx = -INFINITY;
    for (int kj = threadIdx.x; kj < p.Tk; kj += 256) {
        const bf16* kp = p.k + b * p.k_sb + (long)kj * p.k_st + h * p.k_sh;
        float s = 0.f;
        for (int d = 0; d < p.D; ++d) s += qv[d] * bf2f(kp[d]);
        s = s * p.scale + bias_at(p, b, qi, kj);
        if (!visible(p, qi, kj)) s = -INFINITY;
        sc[kj] = s;
        mx = fmaxf(mx, s);
    }
    mx = block_max(mx, red);
    __syncthreads();
    float sum = 0.f;
    const float ms = mx == -INFINITY ? 0.f : mx;
    for (int kj = threadIdx.x; kj < p.Tk; kj += 256) {
        float e = __expf(sc[kj] - ms);
        sc[kj] = e;
        sum += e;
    }
    sum = block_sum(sum, red);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;
    const float rd = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
    if (p.p_drop > 0.f && p.seed_ptr) p.seed = *p.seed_ptr;
    for (int kj = threadIdx.x; kj < p.Tk; kj += 256) {
        float pv = sc[kj] * inv;
        if (p.p_drop > 0.f) pv = hash_uniform(p.seed, drop_idx(p, b, h, qi, kj)) >= p.p_drop ? pv * rd : 0.f;
        sc[kj] = pv;
    }
    __syncthreads();
    bf16* op = p.o + b * p.o_sb + (long)qi * p.o_st + h * p.o_sh;
    for (int d = threadIdx.x; d < p.D; d += 256) {
        float acc = 0.f;
        for (int kj = 0; kj < p.Tk; ++kj) acc += sc[kj] * bf2f(p.v[b * p.v_sb + (long)kj * p.v_st + h * p.v_sh + d]);
        op[d] = f2bf(acc);
    }
    if (threadIdx.x == 0) p.lse[((long)b * p.H + h) * p.Tq + qi] = sum > 0.f ? ms + __logf(sum) : INFINITY;
}

__global__ void __launch_bounds__(256) attn_bwd_generic_k(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* pp = reinterpret_cast<float*>(smem);   // P (undropped)
    float* ds = pp + p.Tk;                          // dS
    float* qv = ds + p.Tk;                          // q row
    float* dov = qv + p.D;                          // dO row
    __shared__ float red[16];
    const int qi = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const bf16* qp = p.q + b * p.q_sb + (long)qi * p.q_st + h * p.q_sh;
    const bf16* dop = p.dout + b * p.do_sb + (long)qi * p.do_st + h * p.do_sh;
    const bf16* op = p.o + b * p.o_sb + (long)qi * p.o_st + h * p.o_sh;
    float dl = 0.f;
    for (int d = threadIdx.x; d < p.D; d += 256) {
        qv[d] = bf2f(qp[d]);
        dov[d] = bf2f(dop[d]);
        dl += dov[d] * bf2f(op[d]);
    }
    dl = block_sum(dl, red);
    const float L = p.lse[((long)b * p.H + h) * p.Tq + qi] * (p.lse_log2 ? LN2 : 1.f);
    const float rd = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
    if (p.p_drop > 0.f && p.seed_ptr) p.seed = *p.seed_ptr;
    for (int kj = threadIdx.x; kj < p.Tk; kj += 256) {
        const bf16* kp = p.k + b * p.k_sb + (long)kj * p.k_st + h * p.k_sh;
        const bf16* vp = p.v + b * p.v_sb + (long)kj * p.v_st + h * p.v_sh;
        float s = 0.f, dp = 0.f;
        for (int d = 0; d < p.D; ++d) { s += qv[d] * bf2f(kp[d]); dp += dov[d] * bf2f(vp[d]); }
        s = s * p.scale + bias_at(p, b, qi, kj);
        float pv = (visible(p, qi, kj) && L != INFINITY) ? __expf(s - L) : 0.f;
        float pd = pv;
        if (p.p_drop > 0.f) {
            bool keep = hash_uniform(p.seed, drop_idx(p, b, h, qi, kj)) >= p.p_drop;
            pd = keep ? pv * rd : 0.f;
            dp = keep ? dp * rd : 0.f;
        }
        pp[kj] = pd;
        ds[kj] = pv * (dp - dl);
    }
    __syncthreads();
    bf16* dqp = p.dq + b * p.dq_sb + (long)qi * p.dq_st + h * p.dq_sh;
    for (int d = threadIdx.x; d < p.D; d += 256) {
        float acc = 0.f;
        for (int kj = 0; kj < p.Tk; ++kj) acc += ds[kj] * bf2f(p.k[b * p.k_sb + (long)kj * p.k_st + h * p.k_sh + d]);
        dqp[d] = f2bf(acc * p.scale);
    }
    // delta for the dK/dV kernel (dK/dV are NOT accumulated here: that took fp32 atomics across
    // query rows, i.e. a run-to-run varying summation order)
    if (threadIdx.x == 0) const_cast<float*>(p.delta)[((long)b * p.H + h) * p.Tq + qi] = dl;
}

// Generic-head-size dK/dV, deterministic: one block per key row j sums over the query rows in a
// fixed order — dVⱼ = Σᵢ P̃ᵢⱼ dOᵢ, dKⱼ = scale · Σᵢ dSᵢⱼ qᵢ with P, dP recomputed from q, k, v, dO,
// the forward's lse and delta = rowsum(dO∘O) written by attn_bwd_generic_k (same dropout mask:
// the hash of the same (b, h, i, j) index).  Scalar (odd head sizes only; 32/64/128 run on MFMA).
__global__ void __launch_bounds__(256) attn_bwd_generic_kv_k(AttnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* pd = reinterpret_cast<float*>(smem);  // P̃ (dropped, rescaled) per query row
    float* ds = pd + p.Tq;                       // dS per query row
    float* kv = ds + p.Tq;                       // k row
    float* vv = kv + p.D;                        // v row
    const int kj = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const bf16* kp = p.k + b * p.k_sb + (long)kj * p.k_st + h * p.k_sh;
    const bf16* vp = p.v + b * p.v_sb + (long)kj * p.v_st + h * p.v_sh;
    for (int d = threadIdx.x; d < p.D; d += 256) {
        kv[d] = bf2f(kp[d]);
        vv[d] = bf2f(vp[d]);
    }
    __syncthreads();
    const float lsc = p.lse_log2 ? LN2 : 1.f;
    const float rd = p.p_drop > 0.f ? 1.f / (1.f - p.p_drop) : 1.f;
    if (p.p_drop > 0.f && p.seed_ptr) p.seed = *p.seed_ptr;
    for (int qi = threadIdx.x; qi < p.Tq; qi += 256) {
        const bf16* qp = p.q + b * p.q_sb + (long)qi * p.q_st + h * p.q_sh;
        const bf16* dop = p.dout + b * p.do_sb + (long)qi * p.do_st + h * p.do_sh;
        const float L = p.lse[((long)b * p.H + h) * p.Tq + qi] * lsc;
        float pv = 0.f, dp = 0.f;
        if (visible(p, qi, kj) && L != INFINITY) {
            float sc = 0.f;
            for (int d = 0; d < p.D; ++d) {
                sc += bf2f(qp[d]) * kv[d];
                dp += bf2f(dop[d]) * vv[d];
            }
            pv = __expf(sc * p.scale + bias_at(p, b, qi, kj) - L);
        }
        float pdv = pv;
        if (p.p_drop > 0.f) {
            const bool keep = hash_uniform(p.seed, drop_idx(p, b, h, qi, kj)) >= p.p_drop;
            pdv = keep ? pv * rd : 0.f;
            dp = keep ? dp * rd : 0.f;
        }
        pd[qi] = pdv;
        ds[qi] = pv * (dp - p.delta[((long)b * p.H + h) * p.Tq + qi]);
    }
    __syncthreads();
    bf16* dkp = p.dk + b * p.dk_sb + (long)kj * p.dk_st + h * p.dk_sh;
    bf16* dvp = p.dv + b * p.dv_sb + (long)kj * p.dv_st + h * p.dv_sh;
    for (int d = threadIdx.x; d < p.D; d += 256) {
        float ak = 0.f, av = 0.f;
        for (int qi = 0; qi < p.Tq; ++qi) {
            const float dsv = ds[qi], pdq = pd[qi];
            if (dsv == 0.f && pdq == 0.f) continue;  // masked (causal / dropped) pairs
            ak += dsv * bf2f(p.q[b * p.q_sb + (long)qi * p.q_st + h * p.q_sh + d]);
            av += pdq * bf2f(p.dout[b * p.do_sb + (long)qi * p.do_st + h * p.do_sh + d]);
        }
        dkp[d] = f2bf(ak * p.scale);
        dvp[d] = f2bf(av);
    }
}

}  // namespace

int attn_launch_fwd_generic(const AttnArgs& a, hipStream_t st) {
    if (a.D > 256 || a.Tk > 12000) return -1;
    return attn_launch((const void*)attn_fwd_generic_k, dim3(a.Tq, a.B * a.H), 256, (a.Tk + a.D) * 4, a, st);
}

int attn_launch_bwd_generic(const AttnArgs& a, hipStream_t st) {
    if (a.D > 256 || a.Tk > 12000 || a.Tq > 12000) return -1;
    const dim3 gq(a.Tq, a.B * a.H), gkv(a.Tk, a.B * a.H);
    const int rc = attn_launch((const void*)attn_bwd_generic_k, gq, 256, (2 * a.Tk + 2 * a.D) * 4, a, st);
    return rc ? rc : attn_launch((const void*)attn_bwd_generic_kv_k, gkv, 256, (2 * a.Tq + 2 * a.D) * 4, a, st);
}

}  // namespace rn_attn
