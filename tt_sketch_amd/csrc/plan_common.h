// What the device headers and the plain-C++ plan headers both read.  No HIP include.
#pragma once
#include <cstdint>

namespace ttsk {

constexpr int SK_MAXB = 32;  // problems of one shape per launch (one tensor of a batch each)

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace ttsk
