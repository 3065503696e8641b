// host_srs_check.hpp -- the host side of the SRS check (include/bbgpu.h, bbgpu_srs_check): the report and the pairing tail -- shared by the GPU entry and
// its host twin, which differ only in who computes the two sums -- and the twin's own O(n) parts (curve test, the sums through the bucket method of
// host_fallback.hpp).  The multipliers, the verdict on x * G2, the pairing and the bisection are host_random_check.hpp's.
// The test: for multipliers rho_i unknown to whoever made the table, A = sum_{i < n-1} rho_i P_i and B = sum_{i < n-1} rho_i P_{i+1} satisfy
// e(A, x G2) = e(B, G2) when P_{i+1} = x P_i for every i, and with probability ~2^-253 otherwise.  It generalises the single pair the reference's
// own test looks at (test/test_io.cpp:12-34: e(-x G, G2) e(G, x G2) = 1) to every row.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_random_check.hpp"

namespace bbgpu {
namespace host {

static inline void srs_report_init(bbgpu_srs_report* R, size_t n, const uint64_t seed[4])
{
    memset(R, 0, sizeof(*R));
    R->n = n;
    R->first_bad_point = UINT64_MAX;
    R->first_bad_power = UINT64_MAX;
    report_no_sums(seed, R->seed, R->a, R->b);
}

// The tail once the curve test has passed, x G2 is good and n >= 2: e(A, x G2) == e(B, G2) through prefix_check.  sums(m, a12, b12): A and B over the first
// m multipliers -- points [0, m) and [1, m + 1).  With BBGPU_SRS_CHECK_LOCATE the first failing prefix ends in the first bad pair.
template <class Sums> static inline int srs_check_powers(bbgpu_srs_report* R, const uint64_t g2_x[16], int flags, Sums sums)
{
    PrefixVerdict v;
    const int rc = prefix_check((size_t)R->n - 1, (flags & BBGPU_SRS_CHECK_LOCATE) != 0, sums,
                                [&](const uint64_t* a12, const uint64_t* b12) { return pair_is_one(a12, b12, g2_x, &G2_ONE); }, &v);
    if (!v.rounds) return rc;
    memcpy(R->a, v.a, 64);
    memcpy(R->b, v.b, 64);
    R->powers_checked = 1;
    R->powers_ok = v.ok ? 1 : 0;
    if (v.first_failing != SIZE_MAX) R->first_bad_power = v.first_failing;
    return rc;
}

// bbgpu_host_srs_check: the same definition over the even entries of a caller's endo table
static inline int srs_check_host(const uint64_t* table, size_t n, const uint64_t* g2_x, const uint64_t seed[4], int flags, bbgpu_srs_report* R)
{
    srs_report_init(R, n, seed);
    const std::vector<uint64_t> rows = canonical_rows(table, n, &R->bad_points, &R->first_bad_point);
    uint64_t gen[8];
    g1_generator_words(gen);
    R->first_is_generator = !memcmp(rows.data(), gen, 64) ? 1 : 0;
    R->g2_ok = srs_check_g2_ok(g2_x) ? 1 : 0;
    if (!R->g2_ok || R->bad_points || n < 2) return BBGPU_OK;
    std::vector<uint64_t> rho((n - 1) * 4);
    fallback_parallel(n - 1, 4096, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) srs_check_rho(seed, i, &rho[4 * i]);
    });
    return srs_check_powers(R, g2_x, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) {
        g1_to_normalised(msm_pippenger(rho.data(), rows.data(), m, 8), a12);
        g1_to_normalised(msm_pippenger(rho.data(), rows.data() + 8, m, 8), b12);
        return (int)BBGPU_OK;
    });
}

} // namespace host
} // namespace bbgpu
