// Per-layout launch of the persistent GEMM (config 9, gemm_pk.h): the epilogue switch shared by the
// static-walk instantiations (gemm_pk_{tt,tf,ft,ff}.hip) and the dynamic-queue ones
// (gemm_pk_{tt,tf,ft,ff}_dyn.hip, separate units so both compile in parallel).  The split-K slab
// reduction that follows a split launch is issued by the static unit's entry point.
#pragma once
#include "gemm_pk.h"


namespace rn_gemm_detail {


// Launches the instance specialised for `form` (gemm_pk.h, PK_EPI_*) if FORMS lists it.
template <bool AK, bool BKC, bool DYN, int ACT, int... FORMS>
bool pk_launch_form(GemmArgs& a, int form, hipStream_t st) {
    bool hit = false;
    ((form == FORMS ? (launch_pk_t<AK, BKC, ACT, false, false, 0, 0, DYN, FORMS>(a, st), hit = true) : false), ...);
    return hit;
}

// The epilogue forms with an instance of their own are the ones the models' training step launches
// (ops/linear.py, ops/loss.py; the tuner times the same launches):
//   x·Wᵀ (forward):  plain, plain with non-temporal stores (the LM head's logits), bias (qkv),
//                    bias + residual (attention projection, fc2), saved-derivative GELU with bias (fc1);
//   dY·W (dgrad):    plain, alpha (the LM head's hidden-state gradient), the multiply by the saved
//                    GELU derivative (fc2's dgrad).
// Every other form runs the PK_EPI_ANY instance of the same kernel below.
template <bool AK, bool BKC, bool DYN>
void pk_launch_layout(GemmArgs& a, int act, hipStream_t st) {
    constexpr bool dgrad = AK && !BKC;  // activation-backward epilogues: dY·W layout only
    constexpr bool fwd = AK && BKC;     // saved-derivative GELU: x·Wᵀ layout only
    if (a.split > 1) {
        launch_pk_t<AK, BKC, ACT_NONE, true, true, 0, false, DYN>(a, st);
        return;
    }
    if (a.out_f32) {
        launch_pk_t<AK, BKC, ACT_NONE, false, true, 0, false, DYN>(a, st);
        return;
    }
    a.st_nt = rn_gemm_st_nt(a);
    const int form = pk_epi_form(a, act);
    if constexpr (fwd) {
        if (act == ACT_NONE && pk_launch_form<AK, BKC, DYN, ACT_NONE, 0, PK_EPI_NT, PK_EPI_BIAS, PK_EPI_BIAS | PK_EPI_RES>(a, form, st))
            return;
        if (act == ACT_GELU_D && pk_launch_form<AK, BKC, DYN, ACT_GELU_D, PK_EPI_BIAS | PK_EPI_PRE>(a, form, st)) return;
    }
    if constexpr (dgrad) {
        if (act == ACT_NONE && pk_launch_form<AK, BKC, DYN, ACT_NONE, 0, PK_EPI_ALPHA>(a, form, st)) return;
        // (the saved-derivative multiply; a specialised ACT_GELU_BWD needs more than 256 VGPRs and spills)
        if (act == ACT_MUL_BWD && a.pre && pk_launch_form<AK, BKC, DYN, ACT_MUL_BWD, 0>(a, form, st)) return;
    }
    switch (act) {
        case ACT_GELU: launch_pk_t<AK, BKC, ACT_GELU, false, false, 0, false, DYN>(a, st); return;
        case ACT_RELU: launch_pk_t<AK, BKC, ACT_RELU, false, false, 0, false, DYN>(a, st); return;
        case ACT_GELU_D:
            if constexpr (fwd) { launch_pk_t<AK, BKC, ACT_GELU_D, false, false, 0, false, DYN>(a, st); return; }
            break;
        case ACT_GELU_BWD:
            if constexpr (dgrad) { launch_pk_t<AK, BKC, ACT_GELU_BWD, false, false, 0, false, DYN>(a, st); return; }
            break;
        case ACT_MUL_BWD:
            if constexpr (dgrad) { launch_pk_t<AK, BKC, ACT_MUL_BWD, false, false, 0, false, DYN>(a, st); return; }
            break;
        case ACT_RELU_BWD:
            if constexpr (dgrad) { launch_pk_t<AK, BKC, ACT_RELU_BWD, false, false, 0, false, DYN>(a, st); return; }
            break;
        default: break;
    }
    launch_pk_t<AK, BKC, ACT_NONE, false, false, 0, false, DYN>(a, st);
}

// the split-K slab reduction + epilogue after a split launch (fixed slab order: deterministic)
inline void pk_splitk_reduce(GemmArgs& a, int act, hipStream_t st) {
    const long total4 = ((long)a.M * a.N + 3) / 4;
    const int g = (int)std::min<long>((total4 + 255) / 256, 4096);
    switch (act) {
        case ACT_GELU: splitk_reduce_k<ACT_GELU><<<g, 256, 0, st>>>(a); break;
        case ACT_GELU_D: splitk_reduce_k<ACT_GELU_D><<<g, 256, 0, st>>>(a); break;
        case ACT_RELU: splitk_reduce_k<ACT_RELU><<<g, 256, 0, st>>>(a); break;
        case ACT_GELU_BWD: splitk_reduce_k<ACT_GELU_BWD><<<g, 256, 0, st>>>(a); break;
        case ACT_MUL_BWD: splitk_reduce_k<ACT_MUL_BWD><<<g, 256, 0, st>>>(a); break;
        case ACT_RELU_BWD: splitk_reduce_k<ACT_RELU_BWD><<<g, 256, 0, st>>>(a); break;
        default:
            splitk_reduce_k<ACT_NONE><<<g, 256, 0, st>>>(a);
            break;
    }
}

}  // namespace rn_gemm_detail

// entry point of one layout: dynamic-queue launch when a counter slot is available (see
// pk_sched_slot), else the static walk; then the split-K reduction
#define RN_PK_ENTRY(NAME, AK, BKC)                                                        \
    void NAME##_dyn(rn_gemm_detail::GemmArgs& a, int act, hipStream_t st);               \
    void NAME(rn_gemm_detail::GemmArgs& a, int act, hipStream_t st) {                    \
        using namespace rn_gemm_detail;                                                   \
        int* slot = pk_sched_slot(a, st);                                                  \
        if (slot) {                                                                       \
            a.sched = slot;                                                               \
            NAME##_dyn(a, act, st);                                                       \
        } else {                                                                          \
            a.sched = nullptr;                                                            \
            pk_launch_layout<AK, BKC, false>(a, act, st);                                 \
        }                                                                                 \
        if (a.split > 1) pk_splitk_reduce(a, act, st);                                    \
    }
#define RN_PK_ENTRY_DYN(NAME, AK, BKC)                                                    \
    void NAME##_dyn(rn_gemm_detail::GemmArgs& a, int act, hipStream_t st) {               \
        rn_gemm_detail::pk_launch_layout<AK, BKC, true>(a, act, st);                      \
    }
