// host_kzg_check_batch.hpp -- the check of up to 2^20 KZG openings by ONE pairing product (include/bbgpu.h: bbgpu_kzg_check_openings,
// bbgpu_kzg_check_open_all and their host twins): the forms a call takes, the verdict on the caller's points, the pairing tail with its bisection --
// shared by the GPU driver (capi.hip) and the twins, which differ only in who computes the rows, the scalars and the two sums -- and the twins' own
// loops.  The definition is host_kzg_check.hpp's, claim by claim:
//   A = sum_t rho_t C_t + (rho_t z_t) pi_t - (sum_t rho_t y_t) G,   B = sum_t rho_t pi_t,   ok = ( e(A, G2) e(-B, x G2) == 1 )
// with C_t = C_{which[t]} collected per shared commitment when the call labels its claims.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_kzg_check.hpp"
#include "host_plonk_verify.hpp"
#include "host_srs_check.hpp"

namespace bbgpu {
namespace host {

// One call in any of its three forms.  Per claim: S == 0, commitments holds count points.  Shared: S commitments, claim t is of commitments[label(t)].
// Open-all: shared, with label(t) = t >> log2n, z_t = omega^(t mod n) and y_t = y[((t >> log2n) * y_stride + t mod n) * 4].
struct KzgCheckCall {
    const uint64_t* commitments = nullptr;
    const uint32_t* which = nullptr; // shared and not open-all
    size_t S = 0;
    const uint64_t* z = nullptr; // null in the open-all form
    const uint64_t* y = nullptr;
    const uint64_t* proofs = nullptr;
    size_t count = 0;
    bool open_all = false;
    int log2n = 0;
    size_t y_stride = 0;

    bool shared() const { return S != 0; }
    size_t head() const { return S + 1; }          // rows of A before the claims' own: the shared commitments, then G
    size_t per() const { return shared() ? 1 : 2; } // rows of a claim: (C_t, pi_t), or pi_t alone
    size_t label(size_t t) const { return open_all ? t >> log2n : which[t]; }
    const uint64_t* y_at(size_t t) const
    {
        if (!open_all) return y + 4 * t;
        const size_t n = (size_t)1 << log2n;
        return y + ((t >> log2n) * y_stride + (t & (n - 1))) * 4;
    }
};

static inline void kzg_report_init(bbgpu_kzg_check_report* R, size_t count, const uint64_t seed[4])
{
    memset(R, 0, sizeof(*R));
    R->count = count;
    R->first_bad = UINT64_MAX;
    R->first_failing = -1;
    R->g2_ok = 1; // a g2_x that is not is refused with the arguments
    report_no_sums(seed, R->seed, R->a, R->b);
}

// The findings among the points.  Shared commitments come first: if one of them is off the curve it is the first finding, by its own index.  Among the
// claims the order is the key 2 t + (1 for the proof): C_t before pi_t (per claim layout), then claim t + 1.
// shared_bad / shared_first: over the S shared commitments (host work on both sides); claims_bad / claims_key: over the claims' own points (~0: none)
static inline void kzg_report_findings(bbgpu_kzg_check_report* R, uint64_t shared_bad, uint64_t shared_first, uint64_t claims_bad, uint64_t claims_key)
{
    R->bad_points = shared_bad + claims_bad;
    if (shared_bad) {
        R->first_bad = shared_first;
        R->first_bad_is_proof = 0;
    } else if (claims_bad) {
        R->first_bad = claims_key >> 1;
        R->first_bad_is_proof = (uint32_t)(claims_key & 1);
    }
}
static inline void kzg_shared_findings(const KzgCheckCall& K, uint64_t* bad, uint64_t* first)
{
    *bad = 0;
    *first = UINT64_MAX;
    for (size_t c = 0; c < K.S; c++)
        if (!g1_words_acceptable(K.commitments + 8 * c) && (*bad)++ == 0) *first = c;
}

// The tail once the points are known to be good, through prefix_check with the verifier's pairing.  sums(m, a12, b12): A and B over the claims [0, m).
// With BBGPU_KZG_CHECK_LOCATE the first failing prefix ends in the first false claim.
template <class Sums> static inline int kzg_check_tail(bbgpu_kzg_check_report* R, const uint64_t g2_x[16], int flags, Sums sums)
{
    PrefixVerdict v;
    const int rc = prefix_check((size_t)R->count, (flags & BBGPU_KZG_CHECK_LOCATE) != 0, sums,
                                [&](const uint64_t* a12, const uint64_t* b12) { return verify_pair(a12, b12, g2_x); }, &v);
    if (!v.rounds) return rc;
    memcpy(R->a, v.a, 64);
    memcpy(R->b, v.b, 64);
    R->rounds = v.rounds;
    R->ok = v.ok ? 1 : 0;
    if (v.first_failing != SIZE_MAX) R->first_failing = (int64_t)v.first_failing;
    return rc;
}

// the argument verdicts every entry gives before anything else: 0, or the code with *why set
static inline int kzg_check_args(const KzgCheckCall& K, bool per_claim_layout, size_t num_commitments, const uint64_t* g2_x, int flags,
                                 const bbgpu_kzg_check_report* out, const char** why)
{
    if (K.count < 1 || K.count > BBGPU_KZG_CHECK_MAX_CLAIMS) {
        *why = "1 .. 2^20 claims are taken";
        return BBGPU_ERR_SIZE;
    }
    if (!K.commitments || !K.y || !K.proofs || (!K.open_all && !K.z) || !g2_x || !out) {
        *why = "null commitments / z / y / proofs / g2_x / report";
        return BBGPU_ERR_ARG;
    }
    if (flags & ~BBGPU_KZG_CHECK_LOCATE) {
        *why = "unknown flag bits";
        return BBGPU_ERR_ARG;
    }
    if (!per_claim_layout && !K.open_all) {
        if (num_commitments < 1 || num_commitments > BBGPU_KZG_CHECK_MAX_COMMITMENTS) {
            *why = "1 .. 64 shared commitments are taken";
            return BBGPU_ERR_ARG;
        }
        for (size_t t = 0; t < K.count; t++)
            if (K.which[t] >= num_commitments) {
                *why = "a label names no commitment";
                return BBGPU_ERR_ARG;
            }
    }
    if (!srs_check_g2_ok(g2_x)) {
        *why = "g2_x is at infinity, off the twist curve or not of order r";
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}
// the sizes of the open-all form: n = 2^k, 1 <= batch <= 64, stride >= n, batch n <= 2^20; *log2n set
static inline bool kzg_check_open_all_sizes_ok(size_t n, size_t stride, int batch, int* log2n)
{
    if (n < 1 || (n & (n - 1)) || batch < 1 || batch > BBGPU_KZG_CHECK_MAX_COMMITMENTS || stride < n || n > BBGPU_KZG_CHECK_MAX_CLAIMS ||
        (size_t)batch * n > BBGPU_KZG_CHECK_MAX_CLAIMS)
        return false;
    int lg = 0;
    while (((size_t)1 << lg) < n) lg++;
    *log2n = lg;
    return true;
}

// a point as a sum takes it (canonical coordinates), or the generator where the flag is set; returns whether it was at infinity
static inline bool kzg_row(const uint64_t* p, uint64_t out[8])
{
    verify_own_point(p, out);
    return g1_words_is_inf(p);
}

// Both twins behind their argument checks; seed: the one in use.  The rows and scalars are laid out as the GPU driver lays them out -- shared: the S
// commitments, G, then pi_t; per claim: G, then (C_t, pi_t) -- so that a prefix of the claims is a prefix of both tables; B reads the same rows from
// the first claim on, with zero on the rows that are commitments.
static inline int kzg_check_host(const KzgCheckCall& K, const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* R)
{
    kzg_report_init(R, K.count, seed);
    const size_t H = K.head(), per = K.per(), count = K.count;
    uint64_t shared_bad, shared_first, claims_bad = 0, claims_key = UINT64_MAX;
    kzg_shared_findings(K, &shared_bad, &shared_first);
    for (size_t t = 0; t < count; t++) {
        if (!K.shared() && !g1_words_acceptable(K.commitments + 8 * t) && claims_bad++ == 0) claims_key = 2 * t;
        if (!g1_words_acceptable(K.proofs + 8 * t) && claims_bad++ == 0) claims_key = 2 * t + 1;
    }
    kzg_report_findings(R, shared_bad, shared_first, claims_bad, claims_key);
    if (R->bad_points) return BBGPU_OK;

    std::vector<uint64_t> pts((H + per * count) * 8), sc_a((H + per * count) * 4, 0), sc_b(per * count * 4, 0);
    std::vector<Fr> rho(count), term(count);
    std::vector<bool> shared_inf(K.S);
    for (size_t c = 0; c < K.S; c++) shared_inf[c] = kzg_row(K.commitments + 8 * c, &pts[8 * c]);
    g1_generator_words(&pts[8 * (H - 1)]);
    const Fr omega = K.open_all ? fr_root_of_unity(K.log2n) : fr_one();
    fallback_parallel(count, 1024, [&](size_t lo, size_t hi) {
        Fr zt = K.open_all ? fr_pow(omega, lo & (((size_t)1 << K.log2n) - 1)) : fr_zero();
        for (size_t t = lo; t < hi; t++) {
            srs_check_rho(seed, t, rho[t].d);
            Fr yt;
            memcpy(yt.d, K.y_at(t), 32);
            if (!K.open_all) memcpy(zt.d, K.z + 4 * t, 32);
            term[t] = fr_mul(yt, rho[t]);
            const size_t row = H + per * t;
            if (!K.shared() && !kzg_row(K.commitments + 8 * t, &pts[8 * row])) memcpy(&sc_a[4 * row], rho[t].d, 32);
            if (!kzg_row(K.proofs + 8 * t, &pts[8 * (row + per - 1)])) {
                const Fr rz = fr_mul(zt, rho[t]);
                memcpy(&sc_a[4 * (row + per - 1)], rz.d, 32);
                memcpy(&sc_b[4 * (per * t + per - 1)], rho[t].d, 32);
            }
            if (K.open_all) zt = fr_mul(zt, omega); // omega^n = 1: the power wraps with the polynomial
        }
    });
    return kzg_check_tail(R, g2_x, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) {
        std::vector<Fr> acc(H, fr_zero());
        for (size_t t = 0; t < m; t++) {
            acc[H - 1] = fr_add(acc[H - 1], term[t]);
            if (K.shared()) acc[K.label(t)] = fr_add(acc[K.label(t)], rho[t]);
        }
        acc[H - 1] = fr_neg(acc[H - 1]);
        for (size_t c = 0; c < K.S; c++)
            if (shared_inf[c]) acc[c] = fr_zero(); // a stand-in row
        memcpy(sc_a.data(), acc.data(), H * 32);
        g1_to_normalised(msm_pippenger(sc_a.data(), pts.data(), H + per * m, 8), a12);
        g1_to_normalised(msm_pippenger(sc_b.data(), pts.data() + 8 * H, per * m, 8), b12);
        return (int)BBGPU_OK;
    });
}

} // namespace host
} // namespace bbgpu
