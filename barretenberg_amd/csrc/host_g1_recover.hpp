// host_g1_recover.hpp -- the host side of bbgpu_g1_ntt and bbgpu_g1_recover (include/bbgpu.h): the verdicts on the arguments that the GPU entries and the
// host twins share -- the curve test of every point among them -- and the twins' own computation.  A column is n curve points, the values on the size-n
// domain of a "polynomial" whose coefficients are points; the transform is host_srs_lagrange.hpp's g1_transform_host and the decoder is the field decoder of
// host_kzg_recover_cells.hpp at l = 1 with every product v z replaced by a plain double-and-add z * P:
//   E_i = z_i P_i on the present rows, infinity on the missing ones;  P = IFFT(E);  Q = FFT(g^j P_j);  Q_i <- Q_i / z'_i;  D' = IFFT(Q);  D_j = g^-j D'_j
// and the points are a codeword of degree < d iff coefficients [d, count) of D are at infinity.  z and z' by the direct products of
// kzg_recover_vanishing_host, one inversion per z'.  Deliberately NOT the split ladder of g1_ladder.hpp and no batch inversion, so that device and twin
// check each other; affine results are unique and canonical, so they agree bit for bit.  bbgpu_g1_recover_each is the same decoder with a row list, and so a
// z and a z', per column: its verdict and twin are at the end, on the one-column routine of the same-set twin.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdio.h>

#include <atomic>
#include <vector>

#include "host_kzg_recover_cells.hpp"
#include "host_kzg_recover_each.hpp"
#include "host_random_check.hpp"
#include "host_srs_lagrange.hpp"

namespace bbgpu {
namespace host {

constexpr int G1_RECOVER_MAX_LOG2 = KZG_RECOVER_MAX_CELLS_LOG2; // n <= 2^16: the vanishing values cost mu x n products
constexpr size_t G1_RECOVER_MAX_POINTS = (size_t)1 << 20;      // batch x n

// n = 2^k with 1 <= k <= 16 -> k, else -1
static inline int g1_recover_log2(size_t n)
{
    for (int k = 1; k <= G1_RECOVER_MAX_LOG2; k++)
        if (n == (size_t)1 << k) return k;
    return -1;
}
// a point as the entries take it: the flag of infinity alone, or canonical coordinates on the curve
static inline bool g1_recover_point_ok(const uint64_t p[8])
{
    if (g1_words_is_inf(p)) return p[7] == 1ULL << 63 && (p[0] | p[1] | p[2] | p[3] | p[4] | p[5] | p[6]) == 0;
    Fq x, y;
    memcpy(x.d, p, 32);
    memcpy(y.d, p + 4, 32);
    Fq cx = x, cy = y;
    fq_cond_sub_p(cx);
    fq_cond_sub_p(cy);
    return fq_eq(cx, x) && fq_eq(cy, y) && g1_on_curve(x, y);
}
// the first of total points that is not acceptable, or total
static inline size_t g1_recover_first_bad_point(const uint64_t* points, size_t total)
{
    std::atomic<size_t> first(total);
    fallback_parallel(total, 4096, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi && i < first.load(std::memory_order_relaxed); i++)
            if (!g1_recover_point_ok(points + 8 * i)) {
                size_t seen = first.load();
                while (i < seen && !first.compare_exchange_weak(seen, i)) {}
                break;
            }
    });
    return first.load();
}
static inline Xyzz g1_from_words(const uint64_t p[8])
{
    if (g1_words_is_inf(p)) return g1_infinity();
    Xyzz r;
    memcpy(r.x.d, p, 32);
    memcpy(r.y.d, p + 4, 32);
    r.zz = FQ_ONE;
    r.zzz = FQ_ONE;
    return r;
}
static inline void g1_to_words(const Xyzz& p, uint64_t out[8])
{
    uint64_t o[12];
    g1_to_normalised(p, o);
    memcpy(out, o, 64);
}
static inline size_t g1_recover_bitrev(size_t i, int log2n)
{
    size_t r = 0;
    for (int b = 0; b < log2n; b++) r |= ((i >> b) & 1) << (log2n - 1 - b);
    return r;
}

// ---- bbgpu_g1_ntt ---------------------------------------------------------------------------------------------------------------------------------------
// The verdict on a call's arguments in the order of include/bbgpu.h: sizes (BBGPU_ERR_SIZE), then pointers, the kind and the points (BBGPU_ERR_ARG).
static inline int g1_ntt_verdict(const char* what, const uint64_t* points, const void* points_out, size_t n, int batch, int kind, int* log2n, char* why,
                                 size_t why_len)
{
    const int lg = g1_recover_log2(n);
    if (lg < 0 || batch < 1 || (size_t)batch > G1_RECOVER_MAX_POINTS / n) {
        snprintf(why, why_len, "%s: n = %zu must be a power of two between 2 and 2^%d, batch (%d) at least 1 and batch x n at most 2^20", what, n,
                 G1_RECOVER_MAX_LOG2, batch);
        return BBGPU_ERR_SIZE;
    }
    if (!points || !points_out) {
        snprintf(why, why_len, "%s: null points / output", what);
        return BBGPU_ERR_ARG;
    }
    if (kind != BBGPU_FFT && kind != BBGPU_IFFT) {
        snprintf(why, why_len, "%s: kind %d: only BBGPU_FFT and BBGPU_IFFT exist on points (no coset and no constant kinds)", what, kind);
        return BBGPU_ERR_ARG;
    }
    const size_t total = (size_t)batch * n, bad = g1_recover_first_bad_point(points, total);
    if (bad != total) {
        snprintf(why, why_len, "%s: the point at position %zu of column %zu is not on the curve or not canonical", what, bad % n, bad / n);
        return BBGPU_ERR_ARG;
    }
    *log2n = lg;
    return BBGPU_OK;
}
// The twin behind its verdict; points_out may alias points.
static inline void g1_ntt_host(const uint64_t* points, uint64_t* points_out, int log2n, int batch, int kind)
{
    const size_t n = (size_t)1 << log2n;
    Fr winv, ninv;
    srs_lagrange_constants(log2n, &winv, &ninv);
    const Fr root = kind == BBGPU_IFFT ? winv : fr_root_of_unity(log2n);
    std::vector<Xyzz> v(n);
    for (int b = 0; b < batch; b++) {
        const uint64_t* in = points + (size_t)b * n * 8;
        for (size_t j = 0; j < n; j++) v[g1_recover_bitrev(j, log2n)] = g1_from_words(in + 8 * j);
        if (kind == BBGPU_IFFT)
            fallback_parallel(n, 16, [&](size_t lo, size_t hi) {
                for (size_t i = lo; i < hi; i++) v[i] = g1_times_plain(v[i], ninv);
            });
        g1_transform_host(v, log2n, root);
        uint64_t* out = points_out + (size_t)b * n * 8;
        fallback_parallel(n, 64, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) g1_to_words(v[i], out + 8 * i);
        });
    }
}

// ---- bbgpu_g1_recover -----------------------------------------------------------------------------------------------------------------------------------
// The verdict, as kzg_recover_verdict's at coset 1; on BBGPU_OK *S holds the shape (l = 1, m = n) and the missing rows.
static inline int g1_recover_verdict(const char* what, const uint32_t* row, size_t count, const uint64_t* points, size_t n, size_t degree_bound, int batch,
                                     const void* points_out, const void* report, KzgRecoverShape* S, char* why, size_t why_len)
{
    const int lg = g1_recover_log2(n);
    if (lg < 0) {
        snprintf(why, why_len, "%s: n = %zu must be a power of two between 2 and 2^%d", what, n, G1_RECOVER_MAX_LOG2);
        return BBGPU_ERR_SIZE;
    }
    if (degree_bound < 1 || degree_bound > n) {
        snprintf(why, why_len, "%s: degree bound %zu outside 1 .. n = %zu", what, degree_bound, n);
        return BBGPU_ERR_SIZE;
    }
    if (count > n || count < degree_bound) {
        snprintf(why, why_len, "%s: %zu rows: at most n = %zu, and no fewer than the degree bound %zu", what, count, n, degree_bound);
        return BBGPU_ERR_SIZE;
    }
    if (batch < 1 || (size_t)batch > G1_RECOVER_MAX_POINTS / n) {
        snprintf(why, why_len, "%s: batch %d below 1, or batch x n above 2^20", what, batch);
        return BBGPU_ERR_SIZE;
    }
    if (!row || !points || !points_out || !report) {
        snprintf(why, why_len, "%s: null row / points / output / report", what);
        return BBGPU_ERR_ARG;
    }
    std::vector<uint8_t> listed(n, 0);
    for (size_t t = 0; t < count; t++) {
        if (row[t] >= n) {
            snprintf(why, why_len, "%s: row[%zu] = %u is not below n = %zu", what, t, row[t], n);
            return BBGPU_ERR_ARG;
        }
        if (listed[row[t]]) {
            snprintf(why, why_len, "%s: row[%zu] = %u is listed twice", what, t, row[t]);
            return BBGPU_ERR_ARG;
        }
        listed[row[t]] = 1;
    }
    const size_t total = (size_t)batch * count, bad = g1_recover_first_bad_point(points, total);
    if (bad != total) {
        snprintf(why, why_len, "%s: the point at position %zu of column %zu (row %u) is not on the curve or not canonical", what, bad % count, bad / count,
                 row[bad % count]);
        return BBGPU_ERR_ARG;
    }
    S->log2n = lg;
    S->log2l = 0;
    S->n = n;
    S->l = 1;
    S->m = n;
    S->mu = n - count;
    S->missing.clear();
    for (size_t k = 0; k < n; k++)
        if (!listed[k]) S->missing.push_back((uint32_t)k);
    return BBGPU_OK;
}
// per column: the smallest index in [d, count) and the smallest in [count, n) whose coefficient is not at infinity, ~0 for none -> the report
static inline int g1_recover_report_of(const char* what, const uint64_t* first_bad, const uint64_t* first_bug, int batch, size_t mu, bbgpu_g1_recover_report* out,
                                       char* why, size_t why_len)
{
    out->consistent = 1;
    out->first_bad_column = 0;
    out->first_bad_coeff = 0;
    out->missing = mu;
    for (int b = 0; b < batch; b++)
        if (first_bug[b] != ~0ull) {
            snprintf(why, why_len, "%s: coefficient %llu of column %d is not at infinity although the construction makes it so: a bug of this library", what,
                     (unsigned long long)first_bug[b], b);
            return BBGPU_ERR_HIP;
        }
    for (int b = 0; b < batch; b++)
        if (first_bad[b] != ~0ull) {
            out->consistent = 0;
            out->first_bad_column = (uint32_t)b;
            out->first_bad_coeff = first_bad[b];
            break;
        }
    return BBGPU_OK;
}
// slot bitrev(i) of dst <- scalar(i) * source(i) for every i < n; scalar(i) in Montgomery form, brought down to the plain integer the double-and-add reads
template <class Scalar, class Source> static inline void g1_recover_pass(std::vector<Xyzz>& dst, int log2n, Scalar scalar, Source source)
{
    const size_t n = (size_t)1 << log2n;
    fallback_parallel(n, 16, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) dst[g1_recover_bitrev(i, log2n)] = g1_times_plain(source(i), fr_from_mont(scalar(i)));
    });
}
// one column: in[t] is the point of row[t]; all n points to out; *first_bad, *first_bug as g1_recover_report_of takes them
static inline void g1_recover_column(const KzgRecoverShape& S, const std::vector<Fr>& z, const std::vector<Fr>& zc_inv, const std::vector<Fr>& gp,
                                     const std::vector<Fr>& gpi, const uint32_t* row, size_t count, const uint64_t* in, size_t degree_bound, uint64_t* out,
                                     uint64_t* first_bad, uint64_t* first_bug)
{
    const size_t n = S.n;
    const int lg = S.log2n;
    Fr winv, ninv_plain;
    srs_lagrange_constants(lg, &winv, &ninv_plain);
    const Fr w = fr_root_of_unity(lg), ninv = fr_inv(fr_from_u64((uint64_t)n));
    std::vector<Xyzz> a(n, g1_infinity()), b(n), pts(n, g1_infinity());
    for (size_t t = 0; t < count; t++) pts[row[t]] = g1_from_words(in + 8 * t);
    g1_recover_pass(a, lg, [&](size_t i) { return fr_mul(z[i], ninv); }, [&](size_t i) { return pts[i]; }); // z_i = 0 on the missing rows
    g1_transform_host(a, lg, winv);
    g1_recover_pass(b, lg, [&](size_t j) { return gp[j]; }, [&](size_t j) { return a[j]; });
    g1_transform_host(b, lg, w);
    g1_recover_pass(a, lg, [&](size_t i) { return fr_mul(zc_inv[i], ninv); }, [&](size_t i) { return b[i]; });
    g1_transform_host(a, lg, winv);
    g1_recover_pass(b, lg, [&](size_t j) { return gpi[j]; }, [&](size_t j) { return a[j]; }); // D_j at slot bitrev(j)
    *first_bad = ~0ull;
    *first_bug = ~0ull;
    for (size_t j = degree_bound; j < n; j++) {
        if (g1_is_inf(b[g1_recover_bitrev(j, lg)])) continue;
        uint64_t& first = j < count ? *first_bad : *first_bug;
        if (first == ~0ull) first = j;
    }
    g1_transform_host(b, lg, w);
    fallback_parallel(n, 64, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) g1_to_words(b[i], out + 8 * i);
    });
}
// g^j and g^-j for j < n: the coset shift and the unshift of both twins
static inline void g1_recover_shift_powers(size_t n, std::vector<Fr>& gp, std::vector<Fr>& gpi)
{
    const Fr g = fr_from_limbs(FrHostP::GEN5), ginv = fr_inv(g);
    gp.resize(n);
    gpi.resize(n);
    Fr p = fr_one(), q = fr_one();
    for (size_t j = 0; j < n; j++) {
        gp[j] = p;
        gpi[j] = q;
        p = fr_mul(p, g);
        q = fr_mul(q, ginv);
    }
}
// The twin behind its verdict.  Short columns are dealt to threads whole (their transforms are too small to split), long ones run one after another.
static inline int g1_recover_host(const KzgRecoverShape& S, const uint32_t* row, size_t count, const uint64_t* points, size_t degree_bound, int batch,
                                  uint64_t* points_out, bbgpu_g1_recover_report* report, char* why, size_t why_len)
{
    std::vector<Fr> z, zc_inv;
    kzg_recover_vanishing_host(S, z, zc_inv);
    const size_t n = S.n;
    std::vector<Fr> gp, gpi;
    g1_recover_shift_powers(n, gp, gpi);
    std::vector<uint64_t> first_bad((size_t)batch, ~0ull), first_bug((size_t)batch, ~0ull);
    auto columns = [&](size_t lo, size_t hi) {
        for (size_t b = lo; b < hi; b++)
            g1_recover_column(S, z, zc_inv, gp, gpi, row, count, points + b * count * 8, degree_bound, points_out + b * n * 8, &first_bad[b], &first_bug[b]);
    };
    if (n < 32) fallback_parallel((size_t)batch, 1, columns);
    else columns(0, (size_t)batch);
    return g1_recover_report_of("host g1_recover", first_bad.data(), first_bug.data(), batch, S.mu, report, why, why_len);
}

// ---- bbgpu_g1_recover_each: every column with ITS OWN rows ------------------------------------------------------------------------------------------------
constexpr int G1_RECOVER_EACH_MAX_LOG2 = 12; // BBGPU_G1_RECOVER_EACH_MAX_ROWS: the vanishing values cost sum_b 2 mu_b n products (include/bbgpu.h)
static_assert(BBGPU_G1_RECOVER_EACH_MAX_ROWS == 1u << G1_RECOVER_EACH_MAX_LOG2, "the cap of include/bbgpu.h");

// The verdict, as kzg_recover_each_verdict's at coset 1: sizes (BBGPU_ERR_SIZE; the counts need the offsets, so a null or malformed offset array is found
// on the way and reported as BBGPU_ERR_ARG), then pointers, the row lists and the points (BBGPU_ERR_ARG); `why` names the first offender by column and
// position.  On BBGPU_OK *S holds the shape (l = 1, m = n) and every column's missing rows, ascending.
static inline int g1_recover_each_verdict(const char* what, const uint32_t* row_offsets, const uint32_t* row, const uint64_t* points, size_t n,
                                          size_t degree_bound, int batch, const void* points_out, const void* report, KzgRecoverEachShape* S, char* why,
                                          size_t why_len)
{
    const int lg = g1_recover_log2(n);
    if (lg < 0 || lg > G1_RECOVER_EACH_MAX_LOG2) {
        snprintf(why, why_len, "%s: n = %zu must be a power of two between 2 and 2^%d", what, n, G1_RECOVER_EACH_MAX_LOG2);
        return BBGPU_ERR_SIZE;
    }
    if (degree_bound < 1 || degree_bound > n) {
        snprintf(why, why_len, "%s: degree bound %zu outside 1 .. n = %zu", what, degree_bound, n);
        return BBGPU_ERR_SIZE;
    }
    if (batch < 1 || (size_t)batch > G1_RECOVER_MAX_POINTS / n) {
        snprintf(why, why_len, "%s: batch %d below 1, or batch x n above 2^20", what, batch);
        return BBGPU_ERR_SIZE;
    }
    if (!row_offsets) {
        snprintf(why, why_len, "%s: null row offsets", what);
        return BBGPU_ERR_ARG;
    }
    if (row_offsets[0] != 0) {
        snprintf(why, why_len, "%s: row_offsets[0] = %u is not 0", what, row_offsets[0]);
        return BBGPU_ERR_ARG;
    }
    for (int b = 0; b < batch; b++)
        if (row_offsets[b + 1] < row_offsets[b]) {
            snprintf(why, why_len, "%s: column %d: row_offsets[%d] = %u is below row_offsets[%d] = %u", what, b, b + 1, row_offsets[b + 1], b, row_offsets[b]);
            return BBGPU_ERR_ARG;
        }
    for (int b = 0; b < batch; b++) {
        const size_t count = row_offsets[b + 1] - row_offsets[b];
        if (count > n || count < degree_bound) {
            snprintf(why, why_len, "%s: column %d lists %zu rows: at most n = %zu, and no fewer than the degree bound %zu", what, b, count, n, degree_bound);
            return BBGPU_ERR_SIZE;
        }
    }
    if (!row || !points || !points_out || !report) {
        snprintf(why, why_len, "%s: null row / points / output / report", what);
        return BBGPU_ERR_ARG;
    }
    S->missing.assign((size_t)batch, std::vector<uint32_t>());
    S->max_missing = 0;
    std::vector<uint8_t> listed(n);
    for (int b = 0; b < batch; b++) {
        const uint32_t* r = row + row_offsets[b];
        const size_t count = row_offsets[b + 1] - row_offsets[b];
        std::fill(listed.begin(), listed.end(), (uint8_t)0);
        for (size_t t = 0; t < count; t++) {
            if (r[t] >= n) {
                snprintf(why, why_len, "%s: column %d: row[%zu] = %u (position %zu of its list) is not below n = %zu", what, b, row_offsets[b] + t, r[t], t, n);
                return BBGPU_ERR_ARG;
            }
            if (listed[r[t]]) {
                snprintf(why, why_len, "%s: column %d: row[%zu] = %u (position %zu of its list) is listed twice", what, b, row_offsets[b] + t, r[t], t);
                return BBGPU_ERR_ARG;
            }
            listed[r[t]] = 1;
        }
        std::vector<uint32_t>& K = S->missing[(size_t)b];
        K.reserve(n - count);
        for (size_t k = 0; k < n; k++)
            if (!listed[k]) K.push_back((uint32_t)k);
        S->max_missing = std::max(S->max_missing, K.size());
    }
    const size_t total = row_offsets[batch], bad = g1_recover_first_bad_point(points, total);
    if (bad != total) {
        int b = 0;
        while (row_offsets[b + 1] <= bad) b++; // the column that owns point `bad`: empty columns cannot (count_b >= degree_bound >= 1 anyway)
        snprintf(why, why_len, "%s: the point at position %zu of column %d (row %u) is not on the curve or not canonical", what, bad - row_offsets[b], b, row[bad]);
        return BBGPU_ERR_ARG;
    }
    S->log2n = lg;
    S->log2l = 0;
    S->n = n;
    S->l = 1;
    S->m = n;
    S->total = total;
    return BBGPU_OK;
}
// per column: the smallest index in [d, count_b) and the smallest in [count_b, n) whose coefficient is not at infinity, ~0 for none -> the report and
// first_bad_out (null or batch); the second kind is BBGPU_ERR_HIP with its text, nothing written
static inline int g1_recover_each_report_of(const char* what, const uint64_t* first_bad, const uint64_t* first_bug, int batch, size_t max_missing,
                                            uint64_t* first_bad_out, bbgpu_g1_recover_each_report* out, char* why, size_t why_len)
{
    for (int b = 0; b < batch; b++)
        if (first_bug[b] != ~0ull) {
            snprintf(why, why_len, "%s: coefficient %llu of column %d is not at infinity although the construction makes it so: a bug of this library", what,
                     (unsigned long long)first_bug[b], b);
            return BBGPU_ERR_HIP;
        }
    out->consistent = 1;
    out->first_bad_column = 0;
    out->first_bad_coeff = 0;
    out->max_missing = max_missing;
    for (int b = batch - 1; b >= 0; b--) {
        if (first_bad_out) first_bad_out[b] = first_bad[b];
        if (first_bad[b] != ~0ull) {
            out->consistent = 0;
            out->first_bad_column = (uint32_t)b;
            out->first_bad_coeff = first_bad[b];
        }
    }
    return BBGPU_OK;
}
// The twin behind its verdict: g1_recover_column once per column with that column's rows, z and z' by direct products over ITS missing rows.  Short
// columns are dealt to threads whole, as in g1_recover_host.
static inline int g1_recover_each_host(const KzgRecoverEachShape& S, const uint32_t* row_offsets, const uint32_t* row, const uint64_t* points, size_t degree_bound,
                                       int batch, uint64_t* points_out, uint64_t* first_bad_out, bbgpu_g1_recover_each_report* report, char* why, size_t why_len)
{
    const size_t n = S.n;
    std::vector<Fr> gp, gpi;
    g1_recover_shift_powers(n, gp, gpi);
    std::vector<uint64_t> first_bad((size_t)batch, ~0ull), first_bug((size_t)batch, ~0ull);
    auto columns = [&](size_t lo, size_t hi) {
        KzgRecoverShape P; // the shape of one column, as the same-set twin sees it
        P.log2n = S.log2n;
        P.log2l = 0;
        P.n = P.m = n;
        P.l = 1;
        std::vector<Fr> z, zc_inv;
        for (size_t b = lo; b < hi; b++) {
            P.missing = S.missing[b];
            P.mu = P.missing.size();
            kzg_recover_vanishing_host(P, z, zc_inv);
            g1_recover_column(P, z, zc_inv, gp, gpi, row + row_offsets[b], row_offsets[b + 1] - row_offsets[b], points + (size_t)row_offsets[b] * 8, degree_bound,
                              points_out + b * n * 8, &first_bad[b], &first_bug[b]);
        }
    };
    if (n < 32) fallback_parallel((size_t)batch, 1, columns);
    else columns(0, (size_t)batch);
    return g1_recover_each_report_of("host g1_recover_each", first_bad.data(), first_bug.data(), batch, S.max_missing, first_bad_out, report, why, why_len);
}

} // namespace host
} // namespace bbgpu
