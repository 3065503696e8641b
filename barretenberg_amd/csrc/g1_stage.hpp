// g1_stage.hpp -- the radix-2 butterfly stage on curve points, the one text srs_lagrange.hip (the inverse transform of bbgpu_srs_lagrange) and
// kzg_open_cosets.hip (both transforms of bbgpu_kzg_open_cosets_device and, at coset size 1, of bbgpu_kzg_open_all_device) launch: decimation in time on
// scratch points (XYZZ, 128 bytes each, ZZ == 0 for infinity; g1_ladder.hpp), one lane per butterfly, the twiddle made in the lane from the root the
// caller passes.  Each including file gets its own copy of the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "g1_ladder.hpp"

namespace bbgpu {

namespace {

constexpr int LT = 64;         // threads per workgroup of the ladder kernels: one wave, as k_srs_update
constexpr int LAGRANGE_WB = 3; // the windows of k_srs_update (srs_update.hip)

// stage s (half = 2^s): butterfly u of n / 2 owns slots g 2 half + pos and that + half, with the twiddle root^(pos n / (2 half)); root261 is a primitive
// n-th root of unity or its inverse, Montgomery-261.  While a stage has at least a wave of groups, consecutive lanes take consecutive GROUPS at one position:
// the twiddle, and with it the skip of the ladder at pos == 0, is wave-uniform (every slot is 128 bytes, so neither order coalesces).  Later stages take
// consecutive positions of one group.  blockIdx.y is the transform of a batch: its n slots start batch_stride slots after those of the one before.
__global__ void __launch_bounds__(LT) k_lagrange_stage(uint32_t* __restrict__ scratch, uint32_t n, uint32_t log2n, uint32_t s, Limbs9 root261, size_t batch_stride)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n / 2) return;
    scratch += (size_t)blockIdx.y * batch_stride * 32;
    const uint32_t half = 1u << s, groups = n >> (s + 1);
    uint32_t pos, g;
    if (groups >= (uint32_t)LT) {
        pos = u >> (log2n - 1 - s); // < half
        g = u & (groups - 1);
    } else {
        pos = u & (half - 1);
        g = u >> s; // < groups
    }
    const size_t ia = (size_t)g * 2 * half + pos, ib = ia + half; // ib <= (groups - 1) 2 half + 2 half - 1 = n - 1
    const uint32_t e = pos * groups;                              // < n / 2
    uint64_t k[4] = { 1, 0, 0, 0 };
    if (e) {
        Fe<FrP, 1, 2> w = fe_one<FrP>(), b = fe_from<FrP>(root261.d);
        for (uint32_t x = e; x; x >>= 1) {
            if (x & 1) w = mul(w, b);
            b = sqr(b);
        }
        FeT<FrP> one_raw = fe_zero<FrP>();
        one_raw.d[0] = 1;
        uint32_t kw[8];
        to_canonical(mul(w, one_raw), kw);
#pragma unroll
        for (int t = 0; t < 4; t++) k[t] = (uint64_t)kw[2 * t] | ((uint64_t)kw[2 * t + 1] << 32);
    }
    butterfly_slots<LAGRANGE_WB>(scratch + ia * 32, scratch + ib * 32, k, e == 0);
}

} // namespace

} // namespace bbgpu
