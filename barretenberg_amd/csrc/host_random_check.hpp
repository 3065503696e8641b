// host_random_check.hpp -- what a random-combination check is, once: the call's seed and the multipliers drawn from it, the verdict on x * G2, the product of
// two pairings every such check ends in, the prefix bisection that names the first failing item, and the canonical rows with their curve test.
// The checks built on it -- bbgpu_srs_check (host_srs_check.hpp), bbgpu_srs_lagrange_check (host_srs_lagrange_check.hpp), the batched PLONK verifier
// (host_plonk_verify.hpp), the KZG checks (host_kzg_check_batch.hpp) and the proof of an SRS update (host_srs_update.hpp) -- fold their items with
// multipliers rho_i unknown to whoever made them into two sums A and B and test ONE relation between the two; the GPU entries and the host twins differ
// only in who computes the sums.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>
#include <sys/random.h>

#include <vector>

#include "../../include/bbgpu.h"
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

// what a report says before any sums are taken: the seed in use, A and B the point at infinity
static inline void report_no_sums(const uint64_t seed[4], uint64_t seed_out[4], uint64_t a[8], uint64_t b[8])
{
    memcpy(seed_out, seed, 32);
    a[7] = b[7] = 1ULL << 63;
}

// g2_x given, no infinity flag, on the twist curve, of order r
static inline bool srs_check_g2_ok(const uint64_t* g2_x)
{
    if (!g2_x) return false;
    if (((g2_x[11] | g2_x[15]) >> 63) & 1) return false;
    const G2Affine q = g2_from_words(g2_x);
    return g2_on_curve(q) && g2_has_order_r(q);
}

// e(a, qa) e(-b, qb) == 1 as one product of two pairings: a and b affine or normalised {x, y, z} (the first 8 words are read, b's y in any representative
// below 2^256), qa and qb 128 bytes each.  A b at infinity is not negated: its flag lives in y.
static inline bool pair_is_one(const uint64_t* a, const uint64_t* b, const void* qa, const void* qb)
{
    uint64_t p[16], q[32];
    memcpy(p, a, 64);
    memcpy(p + 8, b, 64);
    if (!g1_words_is_inf(b)) {
        Fq y;
        memcpy(y.d, b + 4, 32);
        y = fq_neg(fq_canonical(y));
        memcpy(p + 12, y.d, 32);
    }
    memcpy(q, qa, 128);
    memcpy(q + 16, qb, 128);
    return fq12_eq(pairing_product(p, q, 2), fq12_one());
}

// The verdict of a check over `count` items and, when it fails, the first item that makes it fail.
struct PrefixVerdict {
    uint64_t a[12], b[12]; // A and B of the FIRST round: over the whole input
    bool ok;               // that round's verdict
    size_t first_failing;  // SIZE_MAX: none, or not located
    uint32_t rounds;       // the calls of sums that returned 0; 0: not even the first, nothing else here is set
};
// sums(m, a12, b12): A and B over the first m items, normalised; returns BBGPU_OK or the error the entry returns, which ends the check at once.
// accept(a12, b12): the relation between the two.  With `locate` and a failed test the prefix length is bisected: prefix m passes iff every item below m
// is good (up to the soundness error), so the smallest failing prefix ends in the first bad item; at most ceil(log2 count) more rounds.
template <class Sums, class Accept> static inline int prefix_check(size_t count, bool locate, Sums sums, Accept accept, PrefixVerdict* v)
{
    uint64_t a12[12], b12[12];
    v->ok = false;
    v->first_failing = SIZE_MAX;
    v->rounds = 0;
    if (int rc = sums(count, a12, b12)) return rc;
    v->rounds = 1;
    memcpy(v->a, a12, sizeof a12);
    memcpy(v->b, b12, sizeof b12);
    v->ok = accept(a12, b12);
    if (v->ok || !locate) return BBGPU_OK;
    size_t lo = 0, hi = count; // prefix lo passes (the empty one trivially), prefix hi fails
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (int rc = sums(mid, a12, b12)) return rc;
        v->rounds++;
        if (accept(a12, b12)) lo = mid;
        else hi = mid;
    }
    v->first_failing = hi - 1;
    return BBGPU_OK;
}

// canonical affine coordinates on y^2 = x^3 + 3
static inline bool g1_on_curve(const Fq& x, const Fq& y)
{
    return fq_eq(fq_sqr(y), fq_add(fq_mul(fq_sqr(x), x), fq_add(fq_dbl(FQ_ONE), FQ_ONE)));
}
// an affine point as memory holds it (any representative below 2^256) -> canonical coordinates
static inline void g1_words_canonical(const uint64_t p[8], Fq* x, Fq* y)
{
    memcpy(x->d, p, 32);
    memcpy(y->d, p + 4, 32);
    *x = fq_canonical(*x);
    *y = fq_canonical(*y);
}
static inline bool g1_words_on_curve(const uint64_t p[8])
{
    Fq x, y;
    g1_words_canonical(p, &x, &y);
    return g1_on_curve(x, y);
}
// the generator (1, 2), Montgomery
static inline void g1_generator_words(uint64_t out[8])
{
    const Fq gy = fq_dbl(FQ_ONE);
    memcpy(out, FQ_ONE.d, 32);
    memcpy(out + 4, gy.d, 32);
}
// an affine point in the reference's memory format: at infinity (flag), or on the curve
static inline bool g1_words_acceptable(const uint64_t p[8]) { return g1_words_is_inf(p) || g1_words_on_curve(p); }

// The rows as the device keeps them -- canonical, 64 bytes apart -- from the even entries of an endo table.  With `bad` given the rows off the curve are
// counted into it, the first one's index into *first_bad.
static inline std::vector<uint64_t> canonical_rows(const uint64_t* table, size_t n, uint64_t* bad = nullptr, uint64_t* first_bad = nullptr)
{
    std::vector<uint64_t> rows(n * 8);
    for (size_t i = 0; i < n; i++) {
        Fq x, y;
        g1_words_canonical(table + 16 * i, &x, &y);
        memcpy(&rows[8 * i], x.d, 32);
        memcpy(&rows[8 * i + 4], y.d, 32);
        if (bad && !g1_on_curve(x, y) && (*bad)++ == 0) *first_bad = i;
    }
    return rows;
}

} // namespace host
} // namespace bbgpu
