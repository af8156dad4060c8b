// What the device headers and the plain-C++ plan headers both read.  No HIP include.
#pragma once
#include <cstdint>
#include <cstdio>

// How a plan function fails: the reason into the plan's msg, the status to the caller.  `p` is the plan.
#define PLAN_FAIL(status, ...) do { snprintf(p->msg, sizeof(p->msg), __VA_ARGS__); return status; } while (0)

namespace ttsk {

constexpr int SK_MAXB = 32;  // problems of one shape per launch (one tensor of a batch each)
constexpr int64_t PLAN_MAX_EXTENT = (1ll << 31) - 1;  // the kernels index an extent with an int

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

}  // namespace ttsk
