// host_srs_check.hpp -- the host side of the SRS check (include/bbgpu.h, bbgpu_srs_check): the random multipliers, the verdict on x * G2, the
// pairing tail with its bisection -- shared by the GPU entry and its host twin, which differ only in who computes the two sums -- and the twin's
// own O(n) parts (curve test, the sums through the bucket method of host_fallback.hpp).
// The test: for multipliers rho_i unknown to whoever made the table, A = sum_{i < n-1} rho_i P_i and B = sum_{i < n-1} rho_i P_{i+1} satisfy
// e(A, x G2) = e(B, G2) when P_{i+1} = x P_i for every i, and with probability ~2^-253 otherwise.  It generalises the single pair the reference's
// own test looks at (test/test_io.cpp:12-34: e(-x G, G2) e(G, x G2) = 1) to every row.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <sys/random.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_pairing.hpp"
#include "keccak.hpp"

namespace bbgpu {
namespace host {

// rho_i = Keccak-256(seed, 32 bytes, limbs little-endian || i, 8 bytes little-endian) read as four little-endian words, top three bits cleared:
// 253 bits, below r, handed to the MSM as they are (the MSM reads Montgomery form: the effective multiplier is rho_i 2^-256, a bijection of them)
static inline void srs_check_rho(const uint64_t seed[4], uint64_t i, uint64_t out[4])
{
    uint8_t msg[40];
    for (int l = 0; l < 4; l++)
        for (int b = 0; b < 8; b++) msg[8 * l + b] = (uint8_t)(seed[l] >> (8 * b));
    for (int b = 0; b < 8; b++) msg[32 + b] = (uint8_t)(i >> (8 * b));
    keccak256(msg, sizeof msg, out);
    out[3] &= 0x1FFFFFFFFFFFFFFFULL;
}

// the caller's seed, or 32 bytes from the operating system
static inline bool srs_check_seed(const uint64_t* given, uint64_t out[4])
{
    if (given) {
        memcpy(out, given, 32);
        return true;
    }
    size_t got = 0;
    while (got < 32) {
        const ssize_t k = getrandom((uint8_t*)out + got, 32 - got, 0);
        if (k < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        got += (size_t)k;
    }
    return true;
}

static inline void srs_report_init(bbgpu_srs_report* R, size_t n, const uint64_t seed[4])
{
    memset(R, 0, sizeof(*R));
    R->n = n;
    R->first_bad_point = UINT64_MAX;
    R->first_bad_power = UINT64_MAX;
    memcpy(R->seed, seed, 32);
    R->a[7] = R->b[7] = 1ULL << 63; // no sums taken: the point at infinity
}

// g2_x given, no infinity flag, on the twist curve, of order r
static inline bool srs_check_g2_ok(const uint64_t* g2_x)
{
    if (!g2_x) return false;
    if (((g2_x[11] | g2_x[15]) >> 63) & 1) return false;
    const G2Affine q = g2_from_words(g2_x);
    return g2_on_curve(q) && g2_has_order_r(q);
}

// e(A, x G2) == e(B, G2), as one product e(A, x G2) e(-B, G2) == 1; a12 / b12 normalised {x, y, z}
static inline bool srs_check_pair(const uint64_t a12[12], const uint64_t b12[12], const uint64_t g2_x[16])
{
    uint64_t p[16], q[32];
    memcpy(p, a12, 64);
    memcpy(p + 8, b12, 64);
    if (!g1_words_is_inf(b12)) {
        Fq y;
        memcpy(y.d, b12 + 4, 32);
        y = fq_neg(y);
        memcpy(p + 12, y.d, 32);
    }
    memcpy(q, g2_x, 128);
    memcpy(q + 16, &G2_ONE, 128);
    return fq12_eq(pairing_product(p, q, 2), fq12_one());
}

// The tail once the curve test has passed, x G2 is good and n >= 2.  sums(m, a12, b12): A and B over the first m multipliers -- points [0, m) and [1, m + 1) --
// normalised; returns BBGPU_OK or the error the entry returns.  With BBGPU_SRS_CHECK_LOCATE and a failed test the prefix length is bisected: prefix m
// passes iff every pair below m holds (up to the soundness error), so the smallest failing prefix ends in the first bad pair; at most ceil(log2 n) more rounds.
template <class Sums> static inline int srs_check_powers(bbgpu_srs_report* R, const uint64_t g2_x[16], int flags, Sums sums)
{
    uint64_t a12[12], b12[12];
    const size_t pairs = (size_t)R->n - 1;
    if (int rc = sums(pairs, a12, b12)) return rc;
    memcpy(R->a, a12, 64);
    memcpy(R->b, b12, 64);
    R->powers_checked = 1;
    R->powers_ok = srs_check_pair(a12, b12, g2_x) ? 1 : 0;
    if (R->powers_ok || !(flags & BBGPU_SRS_CHECK_LOCATE)) return BBGPU_OK;
    size_t lo = 0, hi = pairs; // prefix lo passes (the empty one trivially), prefix hi fails
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (int rc = sums(mid, a12, b12)) return rc;
        if (srs_check_pair(a12, b12, g2_x)) lo = mid;
        else hi = mid;
    }
    R->first_bad_power = hi - 1;
    return BBGPU_OK;
}

// bbgpu_host_srs_check: the same definition over the even entries of a caller's endo table
static inline int srs_check_host(const uint64_t* table, size_t n, const uint64_t* g2_x, const uint64_t seed[4], int flags, bbgpu_srs_report* R)
{
    srs_report_init(R, n, seed);
    // the rows as the device keeps them: canonical, 64 bytes apart
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
        if (!fq_eq(fq_sqr(y), fq_add(fq_mul(fq_sqr(x), x), three))) {
            if (R->bad_points++ == 0) R->first_bad_point = i;
        }
        if (i == 0) R->first_is_generator = fq_eq(x, FQ_ONE) && fq_eq(y, fq_dbl(FQ_ONE)) ? 1 : 0;
    }
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
