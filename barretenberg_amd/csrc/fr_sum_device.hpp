// fr_sum_device.hpp -- the exact addition the batch sums of the verifiers are made of (plonk_verify.hip k_verify_fold, kzg_check.hip k_kzg_fold):
// canonical 256-bit values modulo r, so that a fixed tree gives the value any other order would.  No floating point, no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fe.hpp"

namespace bbgpu {

__device__ __forceinline__ void fr_add_canonical(uint64_t (&a)[4], const uint64_t (&b)[4])
{
    uint64_t s[4], carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t t = a[i] + b[i];
        const uint64_t c1 = t < a[i];
        s[i] = t + carry;
        carry = c1 | (uint64_t)(s[i] < t);
    }
    uint64_t d[4], borrow = 0; // a + b < 2 r < 2^255: no carry out; subtract r once if it fits
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t t = s[i] - FrP::P64[i];
        const uint64_t b1 = s[i] < FrP::P64[i];
        d[i] = t - borrow;
        borrow = b1 | (uint64_t)(t < borrow);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = borrow ? s[i] : d[i];
}

} // namespace bbgpu
