// host_kzg_open_all.hpp -- the host side of bbgpu_kzg_open_all_* (include/bbgpu.h): the size verdicts and constants the GPU entries and the host twin
// share.  The proofs pi(omega^i) of a polynomial at every point of its domain follow the construction of Feist and Khovratovich: h = the first n entries of
// IDFT_N(DFT_N(s) o DFT_N(t)), N = 2n, s the reversed string and t the coefficients laid out as a Toeplitz column, then the size-n forward transform of
// (h_0 .. h_(n-2), infinity).  That is the coset construction of host_kzg_open_cosets.hpp at coset size 1 without a bound, and the twin is that file's at
// log2l = 0, log2d = log2n (capi.hip bbgpu_host_kzg_open_all).
// Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_srs_lagrange.hpp"

namespace bbgpu {
namespace host {

constexpr int KZG_OPEN_ALL_MAX_LOG2 = 21;       // n; the transforms run at N = 2 n <= 2^22, the limit of the group butterflies (SRS_LAGRANGE_MAX_LOG2)
constexpr int KZG_OPEN_ALL_MAX_BATCH = 64;      // the batch limit of bbgpu_ntt_device_batch
constexpr int KZG_OPEN_ALL_MAX_SLOTS_LOG2 = 22; // batch x 2 n scratch points of 128 bytes: 512 MiB

// n = 2^k with 1 <= k <= 21 -> k, else -1
static inline int kzg_open_all_log2(size_t n)
{
    for (int k = 1; k <= KZG_OPEN_ALL_MAX_LOG2; k++)
        if (n == (size_t)1 << k) return k;
    return -1;
}
// the sizes of one call over a setup of n
static inline bool kzg_open_all_sizes_ok(size_t n, size_t stride_elems, int batch)
{
    return batch >= 1 && batch <= KZG_OPEN_ALL_MAX_BATCH && stride_elems >= n && (size_t)batch * 2 * n <= ((size_t)1 << KZG_OPEN_ALL_MAX_SLOTS_LOG2);
}
static inline size_t bit_reverse(size_t i, int bits)
{
    size_t j = 0;
    for (int b = 0; b < bits; b++) j |= ((i >> b) & 1) << (bits - 1 - b);
    return j;
}
// element i of t, i < 2 n: (c_(n-1), 0 x (n + 1), c_1 .. c_(n-2)) -> the index of the coefficient, or -1 for a zero
static inline long kzg_open_all_t_source(size_t i, size_t n)
{
    if (i == 0) return (long)(n - 1);
    if (i <= n + 1) return -1;
    return (long)(i - n - 1);
}

} // namespace host
} // namespace bbgpu
