// host_kzg_check.hpp -- the check of KZG openings (include/bbgpu.h, bbgpu_host_kzg_check_openings): k claims "the polynomial committed to by C_t takes
// the value y_t at z_t, and pi_t is the commitment of its quotient" hold when
//   e(sum_t rho_t (C_t - y_t G + z_t pi_t), G2) e(-sum_t rho_t pi_t, x G2) == 1
// for multipliers rho_t unknown to whoever made the proofs: each claim alone is e(C - y G + z pi, G2) = e(pi, x G2), i.e. C - y G = (x - z) pi, and a
// random combination of false claims holds with probability ~2^-253.  The multipliers, the seed rule and the verdict on x G2 are bbgpu_srs_check's
// (host_srs_check.hpp); the two sums are one small MSM each (host_fallback.hpp), the pairing side is ONE pairing_product of two pairs.
// Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_pairing.hpp"
#include "host_srs_check.hpp"

namespace bbgpu {
namespace host {

constexpr size_t KZG_CHECK_MAX_OPENINGS = 64;

// an affine point in the reference's memory format: at infinity (flag), or on y^2 = x^3 + 3
static inline bool g1_words_acceptable(const uint64_t p[8])
{
    if (g1_words_is_inf(p)) return true;
    Fq x, y;
    memcpy(x.d, p, 32);
    memcpy(y.d, p + 4, 32);
    x = fq_canonical(x);
    y = fq_canonical(y);
    return fq_eq(fq_sqr(y), fq_add(fq_mul(fq_sqr(x), x), fq_add(fq_dbl(FQ_ONE), FQ_ONE)));
}

// the caller has checked the pointers, k, the points and g2_x; seed: the one in use
static inline bool kzg_check_openings(const uint64_t* commitments, const uint64_t* z, const uint64_t* y, const uint64_t* proofs, size_t k,
                                      const uint64_t g2_x[16], const uint64_t seed[4])
{
    // A = sum_t rho_t C_t + (rho_t z_t) pi_t - (sum_t rho_t y_t) G and B = sum_t rho_t pi_t over plain tables; points at infinity add nothing and are left out
    std::vector<uint64_t> pa, sa, pb, sb;
    auto push = [](std::vector<uint64_t>& pts, std::vector<uint64_t>& sc, const uint64_t* p, const Fr& s) {
        if (g1_words_is_inf(p)) return;
        Fq c[2];
        memcpy(c, p, 64);
        c[0] = fq_canonical(c[0]);
        c[1] = fq_canonical(c[1]);
        pts.insert(pts.end(), c[0].d, c[0].d + 4);
        pts.insert(pts.end(), c[1].d, c[1].d + 4);
        sc.insert(sc.end(), s.d, s.d + 4);
    };
    Fr ysum = fr_zero();
    for (size_t t = 0; t < k; t++) {
        Fr rho, zt, yt;
        srs_check_rho(seed, t, rho.d);
        memcpy(zt.d, z + 4 * t, 32);
        memcpy(yt.d, y + 4 * t, 32);
        push(pa, sa, commitments + 8 * t, rho);
        push(pa, sa, proofs + 8 * t, fr_mul(rho, zt));
        push(pb, sb, proofs + 8 * t, rho);
        ysum = fr_add(ysum, fr_mul(rho, yt));
    }
    uint64_t g[8];
    const Fq gy = fq_dbl(FQ_ONE);
    memcpy(g, FQ_ONE.d, 32);
    memcpy(g + 4, gy.d, 32);
    push(pa, sa, g, fr_neg(ysum));
    uint64_t a12[12], b12[12], p[16], q[32];
    g1_to_normalised(msm_pippenger(sa.data(), pa.data(), sa.size() / 4, 8), a12);
    g1_to_normalised(msm_pippenger(sb.data(), pb.data(), sb.size() / 4, 8), b12);
    memcpy(p, a12, 64);
    memcpy(p + 8, b12, 64);
    if (!g1_words_is_inf(b12)) {
        Fq by;
        memcpy(by.d, b12 + 4, 32);
        by = fq_neg(by);
        memcpy(p + 12, by.d, 32);
    }
    memcpy(q, &G2_ONE, 128);
    memcpy(q + 16, g2_x, 128);
    return fq12_eq(pairing_product(p, q, 2), fq12_one());
}

} // namespace host
} // namespace bbgpu
