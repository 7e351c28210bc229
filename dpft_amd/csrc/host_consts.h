// Host-side constants shared by every translation unit and by the pure host headers (conv_plan.h); no HIP here.
#pragma once
#include <stdint.h>

namespace dpft {

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

constexpr int kNumCU = 256;   // MI355X
constexpr int kNumXCD = 8;

}  // namespace dpft
