// host_srs_lagrange_check.hpp -- the host side of the Lagrange-table check (include/bbgpu.h, bbgpu_srs_lagrange_check): the verdict and its bisection,
// shared by the GPU entry and its host twin, which differ only in who computes the two sums, and the twin's own O(n) parts (the curve loop of
// srs_check_host, the transform and the bucket method of host_fallback.hpp).
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
    memcpy(R->seed, seed, 32);
    R->a[7] = R->b[7] = 1ULL << 63; // no sums taken: the point at infinity
}

// two normalised points {x, y, z}: both infinity, or the same affine coordinates
static inline bool srs_lagrange_check_same(const uint64_t a12[12], const uint64_t b12[12])
{
    const bool ia = g1_words_is_inf(a12), ib = g1_words_is_inf(b12);
    if (ia || ib) return ia && ib;
    return !memcmp(a12, b12, 64);
}

// The tail once the curve test has passed.  sums(m, a12, b12): A over the first m multipliers and rows, B over the transform of the multipliers with
// entries from m on zeroed, against all n rows of the string; normalised; returns BBGPU_OK or the error the entry returns.  With
// BBGPU_SRS_LAGRANGE_CHECK_LOCATE and a failed test the prefix length is bisected: prefix m passes iff every row below m is right (up to the soundness
// error), so the smallest failing prefix ends in the first bad row; at most ceil(log2 n) more rounds.
template <class Sums> static inline int srs_lagrange_check_basis(bbgpu_srs_lagrange_check_report* R, int flags, Sums sums)
{
    uint64_t a12[12], b12[12];
    const size_t n = (size_t)R->n;
    if (int rc = sums(n, a12, b12)) return rc;
    memcpy(R->a, a12, 64);
    memcpy(R->b, b12, 64);
    R->basis_checked = 1;
    R->basis_ok = srs_lagrange_check_same(a12, b12) ? 1 : 0;
    if (R->basis_ok || !(flags & BBGPU_SRS_LAGRANGE_CHECK_LOCATE)) return BBGPU_OK;
    size_t lo = 0, hi = n; // prefix lo passes (the empty one trivially), prefix hi fails
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (int rc = sums(mid, a12, b12)) return rc;
        if (srs_lagrange_check_same(a12, b12)) lo = mid;
        else hi = mid;
    }
    R->first_bad_row = hi - 1;
    return BBGPU_OK;
}

// canonical rows, 64 bytes apart, from the even entries of an endo table; counts the rows off the curve when R is given
static inline std::vector<uint64_t> srs_lagrange_check_rows(const uint64_t* table, size_t n, bbgpu_srs_lagrange_check_report* R)
{
    std::vector<uint64_t> rows(n * 8);
    const Fq three = fq_add(fq_dbl(FQ_ONE), FQ_ONE);
    for (size_t i = 0; i < n; i++) {
        Fq x, y;
        memcpy(x.d, table + 16 * i, 32);
        memcpy(y.d, table + 16 * i + 4, 32);
        x = fq_canonical(x);
        y = fq_canonical(y);
        memcpy(&rows[8 * i], x.d, 32);
        memcpy(&rows[8 * i + 4], y.d, 32);
        if (R && !fq_eq(fq_sqr(y), fq_add(fq_mul(fq_sqr(x), x), three))) {
            if (R->bad_points++ == 0) R->first_bad_point = i;
        }
    }
    return rows;
}

// bbgpu_host_srs_lagrange_check: the same definition over the even entries of two endo tables; n = 2^log2n
static inline int srs_lagrange_check_host(const uint64_t* lagrange, const uint64_t* monomial, size_t n, int log2n, const uint64_t seed[4], int flags,
                                          bbgpu_srs_lagrange_check_report* R)
{
    srs_lagrange_check_report_init(R, n, seed);
    const std::vector<uint64_t> lrows = srs_lagrange_check_rows(lagrange, n, R);
    if (R->bad_points) return BBGPU_OK;
    const std::vector<uint64_t> prows = srs_lagrange_check_rows(monomial, n, nullptr);
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
