// host_srs_lagrange.hpp -- the host side of the Lagrange-basis conversion (include/bbgpu.h, bbgpu_srs_lagrange): the argument verdict and the constants
// the GPU entry and its host twin share (omega_n^-1, n^-1), and the twin's own rows: a curve loop, then a plain radix-2 inverse transform over the points on
// host_g1.hpp with a plain double-and-add per twiddle -- deliberately NOT the split ladder of g1_ladder.hpp, so that the two check each other bit for bit.
// Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_srs_update.hpp"

namespace bbgpu {
namespace host {

constexpr int SRS_LAGRANGE_MAX_LOG2 = 22;

// n = 2^k with 1 <= k <= 22 -> k, else -1
static inline int srs_lagrange_log2(size_t n)
{
    for (int k = 1; k <= SRS_LAGRANGE_MAX_LOG2; k++)
        if (n == (size_t)1 << k) return k;
    return -1;
}
static inline void srs_lagrange_report_init(bbgpu_srs_lagrange_report* R, size_t n)
{
    memset(R, 0, sizeof(*R));
    R->n = n;
    R->first_bad_point = UINT64_MAX;
    R->first_infinity_row = UINT64_MAX;
}
// omega_n^-1 (Montgomery) and n^-1 mod r (a plain integer): what the butterflies and the scaling multiply by
static inline void srs_lagrange_constants(int log2n, Fr* winv, Fr* ninv_plain)
{
    *winv = fr_inv(fr_root_of_unity(log2n));
    *ninv_plain = fr_from_mont(fr_inv(fr_from_u64((uint64_t)1 << log2n)));
}
static inline Xyzz g1_times_plain(const Xyzz& p, const Fr& k)
{
    Xyzz acc = g1_infinity();
    if (g1_is_inf(p)) return acc;
    for (int b = 253; b >= 0; --b) {
        acc = g1_dbl(acc);
        if ((k.d[b >> 6] >> (b & 63)) & 1) acc = g1_add(acc, p);
    }
    return acc;
}

// the radix-2 transform on points, in place: v holds the input in bit-reversed order, root (Montgomery) is a primitive 2^log2n-th root of unity or its
// inverse; out comes sum_j root^(i j) in_j in natural order.  A plain double-and-add per twiddle.  (host_kzg_open_all.hpp runs it both ways.)
static inline void g1_transform_host(std::vector<Xyzz>& v, int log2n, const Fr& root)
{
    const size_t n = (size_t)1 << log2n;
    for (int s = 0; s < log2n; s++) {
        const size_t m = (size_t)1 << s, step = n >> (s + 1); // butterflies (k + j, k + j + m), twiddle root^(j step)
        fallback_parallel(n / 2, 8, [&](size_t lo, size_t hi) {
            for (size_t u = lo; u < hi; u++) {
                const size_t j = u & (m - 1), k = (u >> s) << (s + 1);
                const Xyzz a = v[k + j];
                Xyzz t = v[k + j + m];
                if (j) t = g1_times_plain(t, fr_from_mont(fr_pow(root, (uint64_t)(j * step))));
                Xyzz nt = t;
                nt.y = fq_neg(t.y);
                v[k + j] = g1_add(a, t);
                v[k + j + m] = g1_add(a, nt);
            }
        });
    }
}

// bbgpu_host_srs_lagrange: rows are the even entries of a 2n-entry endo table; table_out may alias table.  n = 2^log2n.
static inline int srs_lagrange_host(const uint64_t* table, size_t n, int log2n, uint64_t* table_out, bbgpu_srs_lagrange_report* R)
{
    // the curve test of canonical_rows (host_random_check.hpp), into bit-reversed slots
    std::vector<Xyzz> v(n);
    for (size_t j = 0; j < n; j++) {
        Fq px, py;
        g1_words_canonical(table + 16 * j, &px, &py);
        if (!g1_on_curve(px, py) && R->bad_points++ == 0) R->first_bad_point = j;
        size_t i = 0;
        for (int b = 0; b < log2n; b++) i |= ((j >> b) & 1) << (log2n - 1 - b);
        v[i] = Xyzz{ px, py, FQ_ONE, FQ_ONE };
    }
    if (R->bad_points) return BBGPU_ERR_ARG;
    Fr winv, ninv;
    srs_lagrange_constants(log2n, &winv, &ninv);
    fallback_parallel(n, 16, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) v[i] = g1_times_plain(v[i], ninv);
    });
    g1_transform_host(v, log2n, winv);
    std::vector<uint64_t> out(16 * n);
    std::vector<uint8_t> inf(n, 0);
    fallback_parallel(n, 64, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; i++) {
            if (g1_is_inf(v[i])) {
                inf[i] = 1;
                continue;
            }
            uint64_t o[12];
            g1_to_normalised(v[i], o);
            Fq x, y;
            memcpy(x.d, o, 32);
            memcpy(y.d, o + 4, 32);
            const Fq bx = fq_mul(x, FQ_BETA), ny = fq_neg(y);
            uint64_t* e = &out[16 * i];
            memcpy(e, x.d, 32);
            memcpy(e + 4, y.d, 32);
            memcpy(e + 8, bx.d, 32);
            memcpy(e + 12, ny.d, 32);
        }
    });
    for (size_t i = 0; i < n; i++)
        if (inf[i] && R->infinity_rows++ == 0) R->first_infinity_row = i;
    if (R->infinity_rows) return BBGPU_ERR_ARG;
    memcpy(table_out, out.data(), 128 * n);
    return BBGPU_OK;
}

} // namespace host
} // namespace bbgpu
