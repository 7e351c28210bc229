// Host-side constants shared by every translation unit and by the pure host headers (conv_plan.h); no HIP here.
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace dpft {

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

constexpr int kNumCU = 256;   // MI355X
constexpr int kNumXCD = 8;

// DPFT_SKIP=family,... (timing experiments, wrong results; README.md): the one switch that conv_plan.h and bn_plan.h both read
inline const char* skip_families() { static const char* s = getenv("DPFT_SKIP"); return s; }

}  // namespace dpft
