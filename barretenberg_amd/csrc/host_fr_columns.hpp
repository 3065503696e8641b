// host_fr_columns.hpp -- the host side of bbgpu_fr_ntt_columns_device and bbgpu_fr_recover_columns_device (include/bbgpu.h): the verdicts on the arguments
// that the GPU entries and the host twins share, and the twins' own computation.  The matrix is row-major, row r at element r stride_elems, and a CODEWORD is
// a column: `rows` values on the size-`rows` domain.  The twin gathers a column, runs the one-polynomial decoder of host_kzg_recover_cells.hpp at l = 1
// over it -- z and z' by the direct products of kzg_recover_vanishing_host, once per SET of rows, the radix-2 transform of host_fallback.hpp -- and writes
// back the rows the column's set misses, nothing else.  It shares no schedule with csrc/fr_columns.hip: no tile, no interleaved transforms, no table of
// multipliers; canonical results are unique, so device and twin agree bit for bit.  Product code, no oracle/; no HIP call, no lock, re-entrant.
#pragma once
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "host_fallback.hpp"
#include "host_kzg_recover_cells.hpp"

namespace bbgpu {
namespace host {

constexpr int FR_COLUMNS_MAX_LOG2 = 11;                        // BBGPU_FR_COLUMNS_MAX_ROWS: a tile of whole columns fits the 2048 LDS elements of a transform
constexpr size_t FR_COLUMNS_MAX_ELEMS = (size_t)1 << 28;       // rows x width
constexpr size_t FR_COLUMNS_MAX_TABLE = (size_t)1 << 20;       // sets x rows: the z tables, the cap of bbgpu_g1_recover_each
static_assert(BBGPU_FR_COLUMNS_MAX_ROWS == 1u << FR_COLUMNS_MAX_LOG2, "the cap of include/bbgpu.h");

// what a verdict leaves for the twin and the driver: the shape, and per set the rows it misses, ascending, in CSR form
struct FrColumnsShape {
    int log2rows = 0;
    size_t rows = 0, width = 0, stride = 0, sets = 0, max_missing = 0;
    std::vector<uint32_t> moff, missing; // sets + 1 offsets into `missing`
};

// rows = 2^k with 1 <= k <= 11 -> k, else -1
static inline int fr_columns_log2(size_t rows)
{
    for (int k = 1; k <= FR_COLUMNS_MAX_LOG2; k++)
        if (rows == (size_t)1 << k) return k;
    return -1;
}
// the sizes of the matrix: BBGPU_ERR_SIZE
static inline int fr_columns_matrix_verdict(const char* what, size_t rows, size_t width, size_t stride_elems, int* log2rows, char* why, size_t why_len)
{
    const int lg = fr_columns_log2(rows);
    if (lg < 0) {
        snprintf(why, why_len, "%s: rows = %zu must be a power of two between 2 and 2^%d", what, rows, FR_COLUMNS_MAX_LOG2);
        return BBGPU_ERR_SIZE;
    }
    if (width < 1 || stride_elems < width || width > FR_COLUMNS_MAX_ELEMS / rows) {
        snprintf(why, why_len, "%s: width %zu below 1, above the stride %zu, or rows x width above 2^28", what, width, stride_elems);
        return BBGPU_ERR_SIZE;
    }
    *log2rows = lg;
    return BBGPU_OK;
}

// ---- bbgpu_fr_ntt_columns_device / bbgpu_host_fr_ntt_columns ----------------------------------------------------------------------------------------------
static inline int fr_ntt_columns_verdict(const char* what, const void* rows_mem, size_t rows, size_t width, size_t stride_elems, int kind, int* log2rows,
                                         char* why, size_t why_len)
{
    if (int rc = fr_columns_matrix_verdict(what, rows, width, stride_elems, log2rows, why, why_len)) return rc;
    if (!rows_mem) {
        snprintf(why, why_len, "%s: null matrix", what);
        return BBGPU_ERR_ARG;
    }
    if (kind != BBGPU_FFT && kind != BBGPU_IFFT) {
        snprintf(why, why_len, "%s: kind %d: only BBGPU_FFT and BBGPU_IFFT exist down a column (no coset and no constant kinds)", what, kind);
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}
// gather, transform, scatter: column by column, dealt to threads in ranges
static inline void fr_ntt_columns_host(uint64_t* m, int log2rows, size_t width, size_t stride_elems, int kind)
{
    const size_t rows = (size_t)1 << log2rows;
    fallback_parallel(width, 16, [&](size_t lo, size_t hi) {
        std::vector<uint64_t> col(4 * rows);
        for (size_t j = lo; j < hi; j++) {
            for (size_t r = 0; r < rows; r++) memcpy(&col[4 * r], m + 4 * (r * stride_elems + j), 32);
            ntt_radix2(col.data(), log2rows, kind, nullptr);
            for (size_t r = 0; r < rows; r++) memcpy(m + 4 * (r * stride_elems + j), &col[4 * r], 32);
        }
    });
}

// ---- bbgpu_fr_recover_columns_device / bbgpu_host_fr_recover_columns --------------------------------------------------------------------------------------
// The verdict in the order of include/bbgpu.h: sizes (BBGPU_ERR_SIZE; the counts need the offsets, so a null or malformed offset array is found on the way
// and reported as BBGPU_ERR_ARG), then pointers and the row lists (BBGPU_ERR_ARG); `why` names the first offender by set and position.
static inline int fr_recover_columns_verdict(const char* what, const uint32_t* set_offsets, const uint32_t* row, int sets, const void* rows_mem, size_t rows,
                                             size_t width, size_t stride_elems, size_t degree_bound, const void* report, FrColumnsShape* S, char* why,
                                             size_t why_len)
{
    int lg;
    if (int rc = fr_columns_matrix_verdict(what, rows, width, stride_elems, &lg, why, why_len)) return rc;
    if (sets < 1 || (size_t)sets > width || (size_t)sets > FR_COLUMNS_MAX_TABLE / rows) {
        snprintf(why, why_len, "%s: sets = %d outside 1 .. width = %zu, or sets x rows above 2^20", what, sets, width);
        return BBGPU_ERR_SIZE;
    }
    if (degree_bound < 1 || degree_bound > rows) {
        snprintf(why, why_len, "%s: degree bound %zu outside 1 .. rows = %zu", what, degree_bound, rows);
        return BBGPU_ERR_SIZE;
    }
    if (!set_offsets) {
        snprintf(why, why_len, "%s: null set offsets", what);
        return BBGPU_ERR_ARG;
    }
    if (set_offsets[0] != 0) {
        snprintf(why, why_len, "%s: set_offsets[0] = %u is not 0", what, set_offsets[0]);
        return BBGPU_ERR_ARG;
    }
    for (int s = 0; s < sets; s++)
        if (set_offsets[s + 1] < set_offsets[s]) {
            snprintf(why, why_len, "%s: set %d: set_offsets[%d] = %u is below set_offsets[%d] = %u", what, s, s + 1, set_offsets[s + 1], s, set_offsets[s]);
            return BBGPU_ERR_ARG;
        }
    for (int s = 0; s < sets; s++) {
        const size_t count = set_offsets[s + 1] - set_offsets[s];
        if (count > rows || count < degree_bound) {
            snprintf(why, why_len, "%s: set %d lists %zu rows: at most rows = %zu, and no fewer than the degree bound %zu", what, s, count, rows, degree_bound);
            return BBGPU_ERR_SIZE;
        }
    }
    if (!row || !rows_mem || !report) {
        snprintf(why, why_len, "%s: null row list / matrix / report", what);
        return BBGPU_ERR_ARG;
    }
    S->moff.assign((size_t)sets + 1, 0);
    S->missing.clear();
    S->max_missing = 0;
    std::vector<uint8_t> listed(rows);
    for (int s = 0; s < sets; s++) {
        const uint32_t* r = row + set_offsets[s];
        const size_t count = set_offsets[s + 1] - set_offsets[s];
        std::fill(listed.begin(), listed.end(), (uint8_t)0);
        for (size_t t = 0; t < count; t++) {
            if (r[t] >= rows) {
                snprintf(why, why_len, "%s: set %d: row[%zu] = %u (position %zu of its list) is not below rows = %zu", what, s, set_offsets[s] + t, r[t], t, rows);
                return BBGPU_ERR_ARG;
            }
            if (listed[r[t]]) {
                snprintf(why, why_len, "%s: set %d: row[%zu] = %u (position %zu of its list) is listed twice", what, s, set_offsets[s] + t, r[t], t);
                return BBGPU_ERR_ARG;
            }
            listed[r[t]] = 1;
        }
        for (size_t k = 0; k < rows; k++)
            if (!listed[k]) S->missing.push_back((uint32_t)k);
        S->moff[(size_t)s + 1] = (uint32_t)S->missing.size();
        S->max_missing = std::max(S->max_missing, rows - count);
    }
    S->log2rows = lg;
    S->rows = rows;
    S->width = width;
    S->stride = stride_elems;
    S->sets = (size_t)sets;
    return BBGPU_OK;
}
// The smallest (column, index) finding of each kind -> the report; bad_column == width: none.  A finding in [count_s, rows) cannot come from any input:
// BBGPU_ERR_HIP and the text, nothing written.
static inline int fr_recover_columns_report_of(const char* what, size_t width, size_t bad_column, uint64_t bad_coeff, size_t bug_column, uint64_t bug_coeff,
                                               size_t max_missing, bbgpu_fr_recover_columns_report* out, char* why, size_t why_len)
{
    if (bug_column < width) {
        snprintf(why, why_len, "%s: coefficient %llu of column %zu is not zero although the construction makes it so: a bug of this library", what,
                 (unsigned long long)bug_coeff, bug_column);
        return BBGPU_ERR_HIP;
    }
    out->consistent = bad_column < width ? 0 : 1;
    out->first_bad_column = bad_column < width ? (uint32_t)bad_column : 0;
    out->first_bad_coeff = bad_column < width ? bad_coeff : 0;
    out->max_missing = max_missing;
    return BBGPU_OK;
}
// The twin behind its verdict.  A failed call (the text above) may have written missing rows, as the device entry may; present rows and the elements at
// [width, stride_elems) are never written.
static inline int fr_recover_columns_host(const FrColumnsShape& S, const uint32_t* set_offsets, const uint32_t* row, uint64_t* m, size_t degree_bound,
                                          uint32_t* first_bad_out, bbgpu_fr_recover_columns_report* report, char* why, size_t why_len)
{
    const size_t rows = S.rows, width = S.width;
    // z and 1 / z' of every set, once
    std::vector<std::vector<Fr>> z(S.sets), zc_inv(S.sets);
    KzgRecoverShape P; // the shape of one column, as the one-polynomial decoder sees it: l = 1, the cells are the rows
    P.log2n = S.log2rows;
    P.log2l = 0;
    P.n = P.m = rows;
    P.l = 1;
    for (size_t s = 0; s < S.sets; s++) {
        P.missing.assign(S.missing.begin() + S.moff[s], S.missing.begin() + S.moff[s + 1]);
        P.mu = P.missing.size();
        kzg_recover_vanishing_host(P, z[s], zc_inv[s]);
    }
    std::vector<uint32_t> bad(width, ~0u), bug(width, ~0u);
    fallback_parallel(width, 8, [&](size_t lo, size_t hi) {
        std::vector<uint64_t> listed(4 * rows), coeffs(4 * rows), values(4 * rows), work(4 * rows);
        for (size_t j = lo; j < hi; j++) {
            const size_t s = j % S.sets, count = set_offsets[s + 1] - set_offsets[s];
            const uint32_t* r = row + set_offsets[s];
            for (size_t t = 0; t < count; t++) memcpy(&listed[4 * t], m + 4 * ((size_t)r[t] * S.stride + j), 32);
            uint64_t b, g;
            kzg_recover_one_host(P, r, count, listed.data(), z[s], zc_inv[s], degree_bound, work, &b, &g, coeffs.data(), values.data());
            bad[j] = b == ~0ull ? ~0u : (uint32_t)b;
            bug[j] = g == ~0ull ? ~0u : (uint32_t)g;
            for (uint32_t k = S.moff[s]; k < S.moff[s + 1]; k++) memcpy(m + 4 * ((size_t)S.missing[k] * S.stride + j), &values[4 * (size_t)S.missing[k]], 32);
        }
    });
    size_t bad_column = width, bug_column = width;
    for (size_t j = width; j-- > 0;) {
        if (bad[j] != ~0u) bad_column = j;
        if (bug[j] != ~0u) bug_column = j;
    }
    bbgpu_fr_recover_columns_report rep;
    if (int rc = fr_recover_columns_report_of("host fr_recover_columns", width, bad_column, bad_column < width ? bad[bad_column] : 0, bug_column,
                                              bug_column < width ? bug[bug_column] : 0, S.max_missing, &rep, why, why_len))
        return rc;
    *report = rep;
    if (first_bad_out) std::copy(bad.begin(), bad.end(), first_bad_out);
    return BBGPU_OK;
}

} // namespace host
} // namespace bbgpu
