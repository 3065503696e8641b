// host_kzg_recover_each.hpp -- the host side of bbgpu_kzg_recover_cells_each (include/bbgpu.h): the verdicts on the arguments that the GPU entry and the
// host twin share, and the twin's own computation -- `batch` polynomials of degree < d, polynomial b rebuilt from ITS OWN count_b of the m = n / l cells.
// Notation and method are host_kzg_recover_cells.hpp's, once per polynomial: with K_b the missing cells of polynomial b the twin computes z_b and z'_b by
// DIRECT products over K_b (kzg_recover_vanishing_host), deliberately not by the product tree of kzg_recover_each.hip, so that it stays an independent
// statement of what the tree must produce.  That costs sum_b mu_b x m x 2 field products: a checker for test sizes, NOT a fallback for m = 2^20 (half
// of 2^20 cells missing would be 2^40 products per polynomial).  Field arithmetic is exact and every output canonical: device and twin agree bit for
// bit.  Product code, no oracle/; no HIP call, no lock, re-entrant.
#pragma once
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "host_kzg_recover_cells.hpp"

namespace bbgpu {
namespace host {

struct KzgRecoverEachShape {
    int log2n = 0, log2l = 0;
    size_t n = 0, l = 0, m = 0, total = 0, max_missing = 0; // total: cell_offsets[batch]
    std::vector<std::vector<uint32_t>> missing;             // per polynomial: the cells that are not listed, ascending
};

// The verdict on a call's arguments, in the order of include/bbgpu.h: sizes (BBGPU_ERR_SIZE; the counts need the offsets, so a null or malformed offset
// array is found on the way and reported as BBGPU_ERR_ARG), then pointers and the cell lists (BBGPU_ERR_ARG); `why` gets the text, which names the first
// offender by polynomial and position.  Nothing is read before it is known to be there; on BBGPU_OK *S holds the shape and the missing cells.
static inline int kzg_recover_each_verdict(const char* what, const uint32_t* cell_offsets, const uint32_t* cell, const void* values, size_t n, size_t coset,
                                           size_t degree_bound, int batch, const void* coeffs_out, size_t stride_elems, const void* report,
                                           KzgRecoverEachShape* S, char* why, size_t why_len)
{
    int log2n, log2l;
    kzg_recover_log2s(n, coset, &log2n, &log2l);
    if (log2n < 0 || log2l < 0 || log2n - log2l < 1) {
        snprintf(why, why_len, "%s: n = %zu must be a power of two between 2 and 2^%d, the coset size (%zu) a power of two between 1 and %d, and n / coset at least 2", what,
                 n, KZG_RECOVER_MAX_LOG2, coset, 1 << KZG_RECOVER_MAX_COSET_LOG2);
        return BBGPU_ERR_SIZE;
    }
    const size_t m = n >> log2l;
    if (degree_bound < 1 || degree_bound > n) {
        snprintf(why, why_len, "%s: degree bound %zu outside 1 .. n = %zu", what, degree_bound, n);
        return BBGPU_ERR_SIZE;
    }
    if (batch < 1 || batch > KZG_RECOVER_MAX_BATCH || stride_elems < n || (size_t)batch * n > KZG_RECOVER_MAX_ELEMS) {
        snprintf(why, why_len, "%s: batch %d outside 1 .. %d, stride %zu below n = %zu, or batch x n above 2^22", what, batch, KZG_RECOVER_MAX_BATCH, stride_elems, n);
        return BBGPU_ERR_SIZE;
    }
    if (!cell_offsets) {
        snprintf(why, why_len, "%s: null cell offsets", what);
        return BBGPU_ERR_ARG;
    }
    if (cell_offsets[0] != 0) {
        snprintf(why, why_len, "%s: cell_offsets[0] = %u is not 0", what, cell_offsets[0]);
        return BBGPU_ERR_ARG;
    }
    for (int b = 0; b < batch; b++)
        if (cell_offsets[b + 1] < cell_offsets[b]) {
            snprintf(why, why_len, "%s: polynomial %d: cell_offsets[%d] = %u is below cell_offsets[%d] = %u", what, b, b + 1, cell_offsets[b + 1], b, cell_offsets[b]);
            return BBGPU_ERR_ARG;
        }
    for (int b = 0; b < batch; b++) {
        const size_t count = cell_offsets[b + 1] - cell_offsets[b];
        if (count < 1 || count > m || count * coset < degree_bound) {
            snprintf(why, why_len, "%s: polynomial %d lists %zu cells of %zu values: at least one, at most n / coset = %zu, and no fewer than the degree bound %zu needs",
                     what, b, count, coset, m, degree_bound);
            return BBGPU_ERR_SIZE;
        }
    }
    if (!cell || !values || !coeffs_out || !report) {
        snprintf(why, why_len, "%s: null cell / values / coefficients / report", what);
        return BBGPU_ERR_ARG;
    }
    S->missing.assign((size_t)batch, std::vector<uint32_t>());
    S->max_missing = 0;
    std::vector<uint8_t> listed(m);
    for (int b = 0; b < batch; b++) {
        const uint32_t* c = cell + cell_offsets[b];
        const size_t count = cell_offsets[b + 1] - cell_offsets[b];
        std::fill(listed.begin(), listed.end(), (uint8_t)0);
        for (size_t t = 0; t < count; t++) {
            if (c[t] >= m) {
                snprintf(why, why_len, "%s: polynomial %d: cell[%zu] = %u (position %zu of its list) is not below n / coset = %zu", what, b, cell_offsets[b] + t, c[t], t, m);
                return BBGPU_ERR_ARG;
            }
            if (listed[c[t]]) {
                snprintf(why, why_len, "%s: polynomial %d: cell[%zu] = %u (position %zu of its list) is listed twice", what, b, cell_offsets[b] + t, c[t], t);
                return BBGPU_ERR_ARG;
            }
            listed[c[t]] = 1;
        }
        std::vector<uint32_t>& K = S->missing[(size_t)b];
        K.reserve(m - count);
        for (size_t k = 0; k < m; k++)
            if (!listed[k]) K.push_back((uint32_t)k);
        S->max_missing = std::max(S->max_missing, K.size());
    }
    S->log2n = log2n;
    S->log2l = log2l;
    S->n = n;
    S->l = coset;
    S->m = m;
    S->total = cell_offsets[batch];
    return BBGPU_OK;
}

// per polynomial: the smallest index in [d, count_b l) and the smallest in [count_b l, n) with a nonzero coefficient, ~0 for none -> the report and
// first_bad_out (null or batch); a nonzero coefficient from count_b l on cannot come from any input: BBGPU_ERR_HIP and the text, nothing written
static inline int kzg_recover_each_report(const char* what, const uint64_t* first_bad, const uint64_t* first_bug, int batch, size_t max_missing,
                                          uint64_t* first_bad_out, bbgpu_kzg_recover_each_report* out, char* why, size_t why_len)
{
    for (int b = 0; b < batch; b++)
        if (first_bug[b] != ~0ull) {
            snprintf(why, why_len, "%s: coefficient %llu of polynomial %d is not zero although the construction makes it so: a bug of this library", what,
                     (unsigned long long)first_bug[b], b);
            return BBGPU_ERR_HIP;
        }
    out->consistent = 1;
    out->first_bad_poly = 0;
    out->first_bad_coeff = 0;
    out->max_missing = max_missing;
    for (int b = batch - 1; b >= 0; b--) {
        if (first_bad_out) first_bad_out[b] = first_bad[b];
        if (first_bad[b] != ~0ull) {
            out->consistent = 0;
            out->first_bad_poly = (uint32_t)b;
            out->first_bad_coeff = first_bad[b];
        }
    }
    return BBGPU_OK;
}

// The twin behind its verdict.  coeffs_out: batch x stride_elems x 4 in host memory, [0, n) of every polynomial written; values_out: null or batch x n x 4;
// first_bad_out: null or batch
static inline int kzg_recover_cells_each_host(const KzgRecoverEachShape& S, const uint32_t* cell_offsets, const uint32_t* cell, const uint64_t* values,
                                              size_t degree_bound, int batch, uint64_t* coeffs_out, size_t stride_elems, uint64_t* values_out,
                                              uint64_t* first_bad_out, bbgpu_kzg_recover_each_report* report, char* why, size_t why_len)
{
    std::vector<uint64_t> first_bad((size_t)batch), first_bug((size_t)batch), work(4 * S.n);
    KzgRecoverShape P; // the shape of one polynomial, as the same-set twin sees it
    P.log2n = S.log2n;
    P.log2l = S.log2l;
    P.n = S.n;
    P.l = S.l;
    P.m = S.m;
    std::vector<Fr> z, zc_inv;
    for (size_t b = 0; b < (size_t)batch; b++) {
        P.missing = S.missing[b];
        P.mu = P.missing.size();
        kzg_recover_vanishing_host(P, z, zc_inv);
        kzg_recover_one_host(P, cell + cell_offsets[b], cell_offsets[b + 1] - cell_offsets[b], values + (size_t)cell_offsets[b] * S.l * 4, z, zc_inv, degree_bound,
                             work, &first_bad[b], &first_bug[b], coeffs_out + b * stride_elems * 4, values_out ? values_out + b * S.n * 4 : nullptr);
    }
    return kzg_recover_each_report("host kzg_recover_cells_each", first_bad.data(), first_bug.data(), batch, S.max_missing, first_bad_out, report, why, why_len);
}

} // namespace host
} // namespace bbgpu
