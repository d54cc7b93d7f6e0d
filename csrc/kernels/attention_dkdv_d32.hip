// Attention backward, dK/dV kernels at head size 32.
#include "attention_bwd_impl.h"

int rn_attn::attn_launch_dkdv_d32(const AttnArgs& a, int groups, unsigned wgs, hipStream_t st) {
    return launch_dkdv<32>(a, groups, wgs, st);
}
