// host_srs_lagrange_check.hpp -- the host side of the Lagrange-table check (include/bbgpu.h, bbgpu_srs_lagrange_check): the verdict and its bisection,
// shared by the GPU entry and its host twin, which differ only in who computes the two sums, and the twin's own O(n) parts (the rows and the bisection of
// host_random_check.hpp, the transform and the bucket method of host_fallback.hpp).
// The test: rows R_i are the Lagrange form L_i = n^-1 sum_j w^(-ij) P_j of the string P iff, for multipliers rho_i unknown to whoever made the table,
//   A = sum_i rho_i R_i   equals   B = sum_j ifft(rho)_j P_j = sum_i rho_i L_i,
// up to the chance 2^-253 that a fixed non-zero combination of the differences R_i - L_i vanishes at random multipliers (the argument of host_srs_check.hpp,
// without its pairing: both sums live in G1).  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_srs_check.hpp"
#include "host_srs_lagrange.hpp"

namespace bbgpu {
namespace host {

static inline void srs_lagrange_check_report_init(bbgpu_srs_lagrange_check_report* R, size_t n, const uint64_t seed[4])
{
    memset(R, 0, sizeof(*R));
    R->n = n;
    R->first_bad_point = UINT64_MAX;
    R->first_bad_row = UINT64_MAX;
    report_no_sums(seed, R->seed, R->a, R->b);
}

// two normalised points {x, y, z}: both infinity, or the same affine coordinates
static inline bool srs_lagrange_check_same(const uint64_t a12[12], const uint64_t b12[12])
{
    const bool ia = g1_words_is_inf(a12), ib = g1_words_is_inf(b12);
    if (ia || ib) return ia && ib;
    return !memcmp(a12, b12, 64);
}

// The tail once the curve test has passed: A == B through prefix_check.  sums(m, a12, b12): A over the first m multipliers and rows, B over the transform
// of the multipliers with entries from m on zeroed, against all n rows of the string.  With BBGPU_SRS_LAGRANGE_CHECK_LOCATE the first failing prefix ends in
// the first bad row.
template <class Sums> static inline int srs_lagrange_check_basis(bbgpu_srs_lagrange_check_report* R, int flags, Sums sums)
{
    PrefixVerdict v;
    const int rc = prefix_check((size_t)R->n, (flags & BBGPU_SRS_LAGRANGE_CHECK_LOCATE) != 0, sums, srs_lagrange_check_same, &v);
    if (!v.rounds) return rc;
    memcpy(R->a, v.a, 64);
    memcpy(R->b, v.b, 64);
    R->basis_checked = 1;
    R->basis_ok = v.ok ? 1 : 0;
    if (v.first_failing != SIZE_MAX) R->first_bad_row = v.first_failing;
    return rc;
}

// bbgpu_host_srs_lagrange_check: the same definition over the even entries of two endo tables; n = 2^log2n
static inline int srs_lagrange_check_host(const uint64_t* lagrange, const uint64_t* monomial, size_t n, int log2n, const uint64_t seed[4], int flags,
                                          bbgpu_srs_lagrange_check_report* R)
{
    srs_lagrange_check_report_init(R, n, seed);
    const std::vector<uint64_t> lrows = canonical_rows(lagrange, n, &R->bad_points, &R->first_bad_point);
    if (R->bad_points) return BBGPU_OK;
    const std::vector<uint64_t> prows = canonical_rows(monomial, n);
    std::vector<uint64_t> rho(n * 4), coef(n * 4);
    fallback_parallel(n, 4096, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) srs_check_rho(seed, i, &rho[4 * i]);
    });
    return srs_lagrange_check_basis(R, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) {
        memcpy(coef.data(), rho.data(), m * 32);
        memset(coef.data() + 4 * m, 0, (n - m) * 32);
        ntt_radix2(coef.data(), log2n, BBGPU_IFFT, nullptr);
        g1_to_normalised(msm_pippenger(rho.data(), lrows.data(), m, 8), a12);
        g1_to_normalised(msm_pippenger(coef.data(), prows.data(), n, 8), b12);
        return (int)BBGPU_OK;
    });
}

} // namespace host
} // namespace bbgpu
