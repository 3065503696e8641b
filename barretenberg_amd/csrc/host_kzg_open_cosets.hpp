// host_kzg_open_cosets.hpp -- the host side of bbgpu_kzg_open_cosets_* (include/bbgpu.h): the size verdicts and constants the GPU entries and the host twin
// share, and the twin's own computation -- the proof pi_k of a polynomial on every coset { omega^(k + m j) : j < l } of its domain, m = n / l, by the
// multi-proof construction of Feist and Khovratovich.  Split the string and the coefficients by residue e = j mod l: P^(e)_b = P_(e + l b),
// c^(e)_a = c_(e + l a).  With M = 2 m and W the M-th root,
//   s^(e) = (P^(e)_(m-2) .. P^(e)_0, infinity x (m + 1)),   t^(e) = (c^(e)_(m-1), 0 x (m + 1), c^(e)_1 .. c^(e)_(m-2)),
//   h = the first m entries of IDFT_M( sum_e DFT_M(s^(e)) o DFT_M(t^(e)) ),
// and the proofs are the size-m forward transform, root omega^l, of (h_0 .. h_(m-2), infinity).  At l = 1 these are the n single proofs, and this twin is the one of
// bbgpu_host_kzg_open_all too (host_kzg_open_all.hpp keeps the verdicts and constants of those entries).  Scalars by
// ntt_radix2, points by g1_transform_host with a plain double-and-add per product and a plain left-to-right sum over e -- NOT the ladder and the lane tree
// of kzg_open_cosets.hip, so that device and twin check each other.
// A polynomial of degree < d, d a power of two with 2 l <= d <= n (bbgpu_kzg_open_cosets_setup_bounded), needs Toeplitz products of size mu = d / l only: with
// M = 2 mu and W the M-th root,
//   s^(e) = (P^(e)_(mu-2) .. P^(e)_0, infinity x (mu + 1)),   t^(e) = (c^(e)_(mu-1), 0 x (mu + 1), c^(e)_1 .. c^(e)_(mu-2)),
//   h = the first mu entries of IDFT_M( sum_e DFT_M(s^(e)) o DFT_M(t^(e)) ),
// and the proofs are the size-m forward transform, root omega^l, of (h_0 .. h_(mu-2), infinity x (m - mu + 1)): rows [0, d - l) and coefficients [0, d) are
// read.  The twin runs ALL log2 m stages of that last transform over the zero-padded input -- NOT the replicating gather of kzg_open_cosets.hip, which
// skips the first log2 (m / mu) of them.  d = n is the construction above, and the entries without a bound are that case.
// Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <algorithm>

#include "host_kzg_open_all.hpp"

namespace bbgpu {
namespace host {

constexpr int KZG_OPEN_COSETS_MAX_COSET_LOG2 = 6; // l <= 64: one wave of kzg_open_cosets.hip sums the l products of a frequency

// n = 2^k, coset = 2^c with 1 <= k <= 21, 0 <= c <= 6 and n / coset >= 2 -> true and the two logarithms
static inline bool kzg_open_cosets_log2(size_t n, size_t coset, int* log2n, int* log2l)
{
    *log2n = kzg_open_all_log2(n);
    *log2l = -1;
    for (int c = 0; c <= KZG_OPEN_COSETS_MAX_COSET_LOG2; c++)
        if (coset == (size_t)1 << c) *log2l = c;
    return *log2n >= 1 && *log2l >= 0 && *log2n - *log2l >= 1;
}
// the degree bound d of a setup of (n, l): a power of two with 2 l <= d <= n -> log2 d, else -1
static inline int kzg_open_cosets_bound_log2(int log2n, int log2l, size_t degree_bound)
{
    for (int k = log2l + 1; k <= log2n; k++)
        if (degree_bound == (size_t)1 << k) return k;
    return -1;
}
// the sizes of one call over a setup of (n, d): kzg_open_all_sizes_ok with the stride held to d, the coefficients that are read
static inline bool kzg_open_cosets_sizes_ok(size_t n, size_t d, size_t stride_elems, int batch)
{
    return kzg_open_all_sizes_ok(n, n, batch) && stride_elems >= d;
}
// element i of t^(e), i < M = 2 m: (c^(e)_(m-1), 0 x (m + 1), c^(e)_1 .. c^(e)_(m-2)) -> the index of the coefficient, or -1 for a zero
static inline long kzg_open_cosets_t_source(size_t i, size_t m, size_t l, size_t e)
{
    const long a = kzg_open_all_t_source(i, m);
    return a < 0 ? -1 : (long)(e + l * (size_t)a);
}

// S^(e) = DFT_M(s^(e)) for every e < l, M = 2 mu = 2 d / l, transform e at S[e M ..], natural order.  Rows [0, d - l) of the table are read (the even
// entries of an endo table); one off the curve: BBGPU_ERR_ARG and the first such index in *bad_row.
static inline int kzg_open_cosets_setup_bounded_host(const uint64_t* table, int log2d, int log2l, std::vector<Xyzz>& S, uint64_t* bad_row)
{
    const int log2M = log2d - log2l + 1;
    const size_t d = (size_t)1 << log2d, l = (size_t)1 << log2l, mu = d >> log2l, M = 2 * mu;
    S.assign(l * M, g1_infinity());
    for (size_t j = 0; j < d - l; j++) { // row j = e + l b, b <= mu - 2
        Fq px, py;
        g1_words_canonical(table + 16 * j, &px, &py);
        if (!g1_on_curve(px, py)) {
            *bad_row = j;
            return BBGPU_ERR_ARG;
        }
        S[(j % l) * M + bit_reverse(mu - 2 - j / l, log2M)] = Xyzz{ px, py, FQ_ONE, FQ_ONE };
    }
    std::vector<Xyzz> v(M);
    for (size_t e = 0; e < l; e++) {
        v.assign(S.begin() + e * M, S.begin() + (e + 1) * M);
        g1_transform_host(v, log2M, fr_root_of_unity(log2M));
        std::copy(v.begin(), v.end(), S.begin() + e * M);
    }
    return BBGPU_OK;
}
// the same without a bound: d = n
static inline int kzg_open_cosets_setup_host(const uint64_t* table, int log2n, int log2l, std::vector<Xyzz>& S, uint64_t* bad_row)
{
    return kzg_open_cosets_setup_bounded_host(table, log2n, log2l, S, bad_row);
}

// the proofs of `batch` polynomials of degree < d over S^ of (d, l): proofs_out[(b m + k) * 8] = the affine pi_k of polynomial b, reference format (infinity:
// bit 63 of y[3], rest zero).  Coefficients [0, d) of every polynomial are read and nothing from d on.
static inline void kzg_open_cosets_proofs_bounded_host(const std::vector<Xyzz>& S, int log2n, int log2l, int log2d, const uint64_t* coeffs, size_t stride_elems,
                                                       int batch, uint64_t* proofs_out)
{
    const int log2m = log2n - log2l, log2mu = log2d - log2l, log2M = log2mu + 1;
    const size_t l = (size_t)1 << log2l, m = (size_t)1 << log2m, mu = (size_t)1 << log2mu, M = 2 * mu;
    const Fr W = fr_root_of_unity(log2M), Minv = fr_inv(fr_from_u64((uint64_t)M));
    std::vector<uint64_t> t(4 * l * M);
    std::vector<Xyzz> v(M), u(m);
    for (int b = 0; b < batch; b++) {
        const uint64_t* c = coeffs + (size_t)b * stride_elems * 4;
        for (size_t e = 0; e < l; e++) {
            uint64_t* te = &t[4 * e * M];
            for (size_t i = 0; i < M; i++) {
                const long src = kzg_open_cosets_t_source(i, mu, l, e); // < d
                if (src < 0) memset(te + 4 * i, 0, 32);
                else memcpy(te + 4 * i, c + 4 * (size_t)src, 32);
            }
            ntt_radix2(te, log2M, BBGPU_FFT, nullptr);
        }
        fallback_parallel(M, 8, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                const size_t j = bit_reverse(i, log2M);
                Xyzz sum = g1_infinity();
                for (size_t e = 0; e < l; e++) {
                    Fr k;
                    memcpy(k.d, &t[4 * (e * M + j)], 32);
                    sum = g1_add(sum, g1_times_plain(S[e * M + j], fr_from_mont(fr_mul(k, Minv))));
                }
                v[i] = sum;
            }
        });
        g1_transform_host(v, log2M, fr_inv(W));
        std::fill(u.begin(), u.end(), g1_infinity()); // h_(mu-1) and everything from mu on: infinity
        for (size_t a = 0; a + 1 < mu; a++) u[bit_reverse(a, log2m)] = v[a];
        g1_transform_host(u, log2m, fr_root_of_unity(log2m)); // all log2 m stages
        uint64_t* out = proofs_out + (size_t)b * m * 8;
        fallback_parallel(m, 64, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                uint64_t o[12];
                g1_to_normalised(u[i], o);
                memcpy(out + 8 * i, o, 64);
            }
        });
    }
}
// the same without a bound: d = n
static inline void kzg_open_cosets_proofs_host(const std::vector<Xyzz>& S, int log2n, int log2l, const uint64_t* coeffs, size_t stride_elems, int batch,
                                               uint64_t* proofs_out)
{
    kzg_open_cosets_proofs_bounded_host(S, log2n, log2l, log2n, coeffs, stride_elems, batch, proofs_out);
}

} // namespace host
} // namespace bbgpu
