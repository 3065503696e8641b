// multi_plan.hpp -- how a host-pointer MSM is cut over the device contexts of bbgpu_init_devices (capi.hip, bbgpu_msm_g1 / bbgpu_msm_g1_batch).
// The point-range split of batched_scalar_multiplications (scalar_multiplication.cpp:703-738), one range per context instead of per thread: context k
// takes points [n k / m, n (k + 1) / m) and the partial sums are added on the host (a sum over a range of points is a plain term of the MSM).
// Host-only and free of HIP, so that a CPU test can compile it on its own.
#pragma once
#include <stddef.h>

namespace bbgpu {
namespace multi {

// No context gets fewer points than this: below it one GPU finishes an MSM in a few launches' time and a second context only adds its own fixed costs.
// Where a split starts to pay has NOT been measured on hardware; this is a floor that keeps every slice a full-size MSM, not a tuned crossover.
constexpr size_t SPLIT_MIN_POINTS = (size_t)1 << 16;

struct Slice {
    int context;
    size_t first, len; // points [first, first + len) of the call
};

// Number of contexts an MSM of n points uses out of `count` bound ones: m = min(count, n / SPLIT_MIN_POINTS), at least 1.
inline int plan_contexts(size_t n, int count)
{
    const size_t by_size = n / SPLIT_MIN_POINTS;
    size_t m = count < 1 ? 1 : (size_t)count;
    if (by_size < m) m = by_size;
    return m < 1 ? 1 : (int)m;
}

// Fills out[0 .. m) with the slices, in context order, tiling [0, n) exactly; returns m.  `out` holds at least `count` entries.
inline int plan_slices(size_t n, int count, Slice* out)
{
    const int m = plan_contexts(n, count);
    for (int k = 0; k < m; k++) {
        const size_t lo = n * (size_t)k / (size_t)m, hi = n * (size_t)(k + 1) / (size_t)m;
        out[k] = Slice{ k, lo, hi - lo };
    }
    return m;
}

} // namespace multi
} // namespace bbgpu
