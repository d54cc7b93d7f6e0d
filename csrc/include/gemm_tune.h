// The measured tile-config / split-K autotuner of the bf16 GEMM (csrc/bindings/gemm_tune.cpp), as
// csrc/bindings/gemm.cpp uses it.
#pragma once
#include <functional>
#include <utility>

#include "gemm_plan.h"

namespace gemm_tune {

// Launches candidate (cfg, split) of the problem being tuned into scratch on the current stream;
// returns rn_gemm's status.
using Trial = std::function<int(int cfg, int split)>;

bool enabled();        // REPLICANN_GEMM_AUTOTUNE=0 disables tuning
bool lib_candidate();  // REPLICANN_GEMM_LIB=1: the vendor library (cfg 7) joins the candidates (A/B runs only)

// the table's (cfg, split) for p, if it has one
bool lookup(const GemmProblem& p, int* cfg, int* split);
// Times gemm_candidates(p) through `trial`, stores the fastest in the table and returns it.
// Never call it while the stream is being captured.
std::pair<int, int> tune(const GemmProblem& p, const Trial& trial);

}  // namespace gemm_tune
