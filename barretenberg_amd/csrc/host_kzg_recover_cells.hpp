// host_kzg_recover_cells.hpp -- the host side of bbgpu_kzg_recover_cells (include/bbgpu.h): the verdicts on the arguments that the GPU entry and the host
// twin share, and the twin's own computation -- `batch` polynomials of degree < d rebuilt from the SAME `count` of their m = n / l cells.  With K the
// missing cells, psi = omega^l and g the coset generator of BBGPU_COSET_FFT, Z = prod_{k in K} (X^l - psi^k) takes the value z_a = prod_k (psi^a - psi^k)
// at every omega^i, i = a mod m, and z'_a = prod_k (g^l psi^a - psi^k) != 0 at g omega^i, so Z never exists in coefficient form:
//   E_i = v_i z_(i mod m) on the present cells, 0 on the missing ones      the values of f Z on the domain, deg f Z < n
//   P = IFFT(E);  Q = COSET_FFT(P);  Q_i *= 1 / z'_(i mod m);  D = COSET_IFFT(Q) = f
// and the cells are values of ONE polynomial of degree < d iff coefficients [d, count l) of D vanish (those from count l on vanish by construction).  Plain
// loops over host_fr.hpp and ntt_radix2 -- one inversion per z', not the batch inversion of poly.hip; one product chain per a, not the tiles and the lane
// tree of kzg_recover_cells.hip -- so that device and twin check each other.  Field arithmetic is exact and every output canonical: they agree bit for
// bit.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdio.h>

#include <vector>

#include "host_fallback.hpp"

namespace bbgpu {
namespace host {

constexpr int KZG_RECOVER_MAX_LOG2 = 21;       // n <= 2^21, as the producers of cell proofs
constexpr int KZG_RECOVER_MAX_COSET_LOG2 = 6;  // l <= 64
constexpr int KZG_RECOVER_MAX_CELLS_LOG2 = 16; // m <= 2^16: the vanishing values cost mu x m products
constexpr int KZG_RECOVER_MAX_BATCH = 64;
constexpr size_t KZG_RECOVER_MAX_ELEMS = (size_t)1 << 22; // batch x n

struct KzgRecoverShape {
    int log2n = 0, log2l = 0;
    size_t n = 0, l = 0, m = 0, mu = 0;
    std::vector<uint32_t> missing; // the mu cells that are not listed, ascending
};

// log2 n and log2 of the coset size where they are powers of two within the limits above, else -1 (both verdicts, each with its own text)
static inline void kzg_recover_log2s(size_t n, size_t coset, int* log2n, int* log2l)
{
    *log2n = *log2l = -1;
    for (int k = 1; k <= KZG_RECOVER_MAX_LOG2; k++)
        if (n == (size_t)1 << k) *log2n = k;
    for (int c = 0; c <= KZG_RECOVER_MAX_COSET_LOG2; c++)
        if (coset == (size_t)1 << c) *log2l = c;
}

// The verdict on a call's arguments, in the order of include/bbgpu.h: sizes (BBGPU_ERR_SIZE), then pointers and the cell list (BBGPU_ERR_ARG); `why`
// gets the text.  Nothing is read before it is known to be there; on BBGPU_OK *S holds the shape and the missing cells.
static inline int kzg_recover_verdict(const char* what, const uint32_t* cell, size_t count, const void* values, size_t n, size_t coset, size_t degree_bound,
                                      int batch, const void* coeffs_out, size_t stride_elems, const void* report, KzgRecoverShape* S, char* why, size_t why_len)
{
    int log2n, log2l;
    kzg_recover_log2s(n, coset, &log2n, &log2l);
    if (log2n < 0 || log2l < 0 || log2n - log2l < 1 || log2n - log2l > KZG_RECOVER_MAX_CELLS_LOG2) {
        snprintf(why, why_len, "%s: n = %zu must be a power of two between 2 and 2^%d, the coset size (%zu) a power of two between 1 and %d, and n / coset between 2 and 2^%d",
                 what, n, KZG_RECOVER_MAX_LOG2, coset, 1 << KZG_RECOVER_MAX_COSET_LOG2, KZG_RECOVER_MAX_CELLS_LOG2);
        return BBGPU_ERR_SIZE;
    }
    const size_t m = n >> log2l;
    if (degree_bound < 1 || degree_bound > n) {
        snprintf(why, why_len, "%s: degree bound %zu outside 1 .. n = %zu", what, degree_bound, n);
        return BBGPU_ERR_SIZE;
    }
    if (count > m || count * coset < degree_bound) {
        snprintf(why, why_len, "%s: %zu cells of %zu values: at most n / coset = %zu, and no fewer than the degree bound %zu needs", what, count, coset, m, degree_bound);
        return BBGPU_ERR_SIZE;
    }
    if (batch < 1 || batch > KZG_RECOVER_MAX_BATCH || stride_elems < n || (size_t)batch * n > KZG_RECOVER_MAX_ELEMS) {
        snprintf(why, why_len, "%s: batch %d outside 1 .. %d, stride %zu below n = %zu, or batch x n above 2^22", what, batch, KZG_RECOVER_MAX_BATCH, stride_elems, n);
        return BBGPU_ERR_SIZE;
    }
    if (!cell || !values || !coeffs_out || !report) {
        snprintf(why, why_len, "%s: null cell / values / coefficients / report", what);
        return BBGPU_ERR_ARG;
    }
    std::vector<uint8_t> listed(m, 0);
    for (size_t t = 0; t < count; t++) {
        if (cell[t] >= m) {
            snprintf(why, why_len, "%s: cell[%zu] = %u is not below n / coset = %zu", what, t, cell[t], m);
            return BBGPU_ERR_ARG;
        }
        if (listed[cell[t]]) {
            snprintf(why, why_len, "%s: cell[%zu] = %u is listed twice", what, t, cell[t]);
            return BBGPU_ERR_ARG;
        }
        listed[cell[t]] = 1;
    }
    S->log2n = log2n;
    S->log2l = log2l;
    S->n = n;
    S->l = coset;
    S->m = m;
    S->mu = m - count;
    S->missing.clear();
    for (size_t k = 0; k < m; k++)
        if (!listed[k]) S->missing.push_back((uint32_t)k);
    return BBGPU_OK;
}

// per polynomial: the smallest index in [d, count l) and the smallest in [count l, n) with a nonzero coefficient, ~0 for none -> the report; a nonzero
// coefficient from count l on cannot come from any input: BBGPU_ERR_HIP and the text
static inline int kzg_recover_report(const char* what, const uint64_t* first_bad, const uint64_t* first_bug, int batch, size_t mu, bbgpu_kzg_recover_report* out,
                                     char* why, size_t why_len)
{
    out->consistent = 1;
    out->first_bad_poly = 0;
    out->first_bad_coeff = 0;
    out->missing = mu;
    for (int b = 0; b < batch; b++)
        if (first_bug[b] != ~0ull) {
            snprintf(why, why_len, "%s: coefficient %llu of polynomial %d is not zero although the construction makes it so: a bug of this library", what,
                     (unsigned long long)first_bug[b], b);
            return BBGPU_ERR_HIP;
        }
    for (int b = 0; b < batch; b++)
        if (first_bad[b] != ~0ull) {
            out->consistent = 0;
            out->first_bad_poly = (uint32_t)b;
            out->first_bad_coeff = first_bad[b];
            break;
        }
    return BBGPU_OK;
}

// z_a (Montgomery) and 1 / z'_a for every a < m
static inline void kzg_recover_vanishing_host(const KzgRecoverShape& S, std::vector<Fr>& z, std::vector<Fr>& zc_inv)
{
    const Fr psi = fr_root_of_unity(S.log2n - S.log2l);
    Fr gl = fr_from_limbs(FrHostP::GEN5);
    for (int i = 0; i < S.log2l; i++) gl = fr_sqr(gl);
    std::vector<Fr> pw(S.m);
    Fr p = fr_one();
    for (size_t a = 0; a < S.m; a++) {
        pw[a] = p;
        p = fr_mul(p, psi);
    }
    z.assign(S.m, fr_one());
    zc_inv.assign(S.m, fr_one());
    fallback_parallel(S.m, 64, [&](size_t lo, size_t hi) {
        for (size_t a = lo; a < hi; a++) {
            const Fr x = pw[a], xc = fr_mul(gl, pw[a]);
            Fr acc = fr_one(), accc = fr_one();
            for (uint32_t k : S.missing) {
                acc = fr_mul(acc, fr_sub(x, pw[k]));
                accc = fr_mul(accc, fr_sub(xc, pw[k]));
            }
            z[a] = acc;
            zc_inv[a] = fr_inv(accc); // never zero: g^n != 1
        }
    });
}

// ONE polynomial of either twin (host_kzg_recover_each.hpp loops over this too): its `count` listed cells and their count x l values, z and 1 / z' of
// ITS missing cells (kzg_recover_vanishing_host) -> the n coefficients at coeffs_out, the n values at values_out unless that is null, and the smallest
// index in [d, count l) and in [count l, n) with a nonzero coefficient (~0 for none).  work: 4 n words of the caller's, overwritten.
static inline void kzg_recover_one_host(const KzgRecoverShape& S, const uint32_t* cell, size_t count, const uint64_t* values, const std::vector<Fr>& z,
                                        const std::vector<Fr>& zc_inv, size_t degree_bound, std::vector<uint64_t>& work, uint64_t* first_bad, uint64_t* first_bug,
                                        uint64_t* coeffs_out, uint64_t* values_out)
{
    const size_t n = S.n, l = S.l, m = S.m, present = count * l;
    const Fr one = fr_one();
    Fr* E = reinterpret_cast<Fr*>(work.data());
    for (size_t i = 0; i < n; i++) E[i] = fr_zero();
    for (size_t t = 0; t < count; t++)
        for (size_t j = 0; j < l; j++) {
            Fr x;
            memcpy(x.d, values + 4 * (t * l + j), 32);
            E[cell[t] + m * j] = fr_mul(fr_mul(x, one), z[cell[t]]); // any representative below 2^256 -> the field
        }
    ntt_radix2(work.data(), S.log2n, BBGPU_IFFT, nullptr);
    ntt_radix2(work.data(), S.log2n, BBGPU_COSET_FFT, nullptr);
    for (size_t i = 0; i < n; i++) E[i] = fr_mul(E[i], zc_inv[i & (m - 1)]);
    ntt_radix2(work.data(), S.log2n, BBGPU_COSET_IFFT, nullptr);
    *first_bad = *first_bug = ~0ull;
    for (size_t i = degree_bound; i < n; i++) {
        if (fr_is_zero(E[i])) continue;
        uint64_t& first = i < present ? *first_bad : *first_bug;
        if (first == ~0ull) first = i;
    }
    memcpy(coeffs_out, work.data(), n * 32);
    if (values_out) {
        ntt_radix2(work.data(), S.log2n, BBGPU_FFT, nullptr);
        memcpy(values_out, work.data(), n * 32);
    }
}

// The twin behind its verdict.  coeffs_out: batch x stride_elems x 4 in host memory, [0, n) of every polynomial written; values_out: null or batch x n x 4
static inline int kzg_recover_cells_host(const KzgRecoverShape& S, const uint32_t* cell, size_t count, const uint64_t* values, size_t degree_bound, int batch,
                                         uint64_t* coeffs_out, size_t stride_elems, uint64_t* values_out, bbgpu_kzg_recover_report* report, char* why,
                                         size_t why_len)
{
    std::vector<Fr> z, zc_inv;
    kzg_recover_vanishing_host(S, z, zc_inv);
    std::vector<uint64_t> first_bad((size_t)batch), first_bug((size_t)batch), work(4 * S.n);
    for (size_t b = 0; b < (size_t)batch; b++)
        kzg_recover_one_host(S, cell, count, values + b * count * S.l * 4, z, zc_inv, degree_bound, work, &first_bad[b], &first_bug[b],
                             coeffs_out + b * stride_elems * 4, values_out ? values_out + b * S.n * 4 : nullptr);
    return kzg_recover_report("host kzg_recover_cells", first_bad.data(), first_bug.data(), batch, S.mu, report, why, why_len);
}

} // namespace host
} // namespace bbgpu
