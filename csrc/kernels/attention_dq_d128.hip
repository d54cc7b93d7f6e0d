// Attention backward, dQ kernels at head size 128.
#include "attention_bwd_impl.h"

int rn_attn::attn_launch_dq_d128(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st) {
    return launch_dq<128>(a, groups, wgs, st);
}
