// Attention backward, dQ kernels at head size 64.
#include "attention_bwd_impl.h"

int rn_attn::attn_launch_dq_d64(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st) {
    return launch_dq<64>(a, groups, wgs, st);
}
