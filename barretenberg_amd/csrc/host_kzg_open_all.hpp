// host_kzg_open_all.hpp -- the host side of bbgpu_kzg_open_all_* (include/bbgpu.h): the size verdicts and constants the GPU entries and the host twin
// share, and the twin's own computation -- the proofs pi(omega^i) of a polynomial at every point of its domain by the construction of Feist and
// Khovratovich: h = the first n entries of IDFT_N(DFT_N(s) o DFT_N(t)), N = 2n, s the reversed string and t the coefficients laid out as a Toeplitz
// column, then the size-n forward transform of (h_0 .. h_(n-2), infinity).  Scalars by ntt_radix2 (host_fallback.hpp), points by the radix-2 transform of
// host_srs_lagrange.hpp with a plain double-and-add per product -- NOT the split ladder of g1_ladder.hpp, so that device and twin check each other.
// Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_srs_lagrange.hpp"

namespace bbgpu {
namespace host {

constexpr int KZG_OPEN_ALL_MAX_LOG2 = 21;       // n; the transforms run at N = 2 n <= 2^22, the limit of the group butterflies (SRS_LAGRANGE_MAX_LOG2)
constexpr int KZG_OPEN_ALL_MAX_BATCH = 64;      // the batch limit of bbgpu_ntt_device_batch
constexpr int KZG_OPEN_ALL_MAX_SLOTS_LOG2 = 22; // batch x 2 n scratch points of 128 bytes: 512 MiB

// n = 2^k with 1 <= k <= 21 -> k, else -1
static inline int kzg_open_all_log2(size_t n)
{
    for (int k = 1; k <= KZG_OPEN_ALL_MAX_LOG2; k++)
        if (n == (size_t)1 << k) return k;
    return -1;
}
// the sizes of one call over a setup of n
static inline bool kzg_open_all_sizes_ok(size_t n, size_t stride_elems, int batch)
{
    return batch >= 1 && batch <= KZG_OPEN_ALL_MAX_BATCH && stride_elems >= n && (size_t)batch * 2 * n <= ((size_t)1 << KZG_OPEN_ALL_MAX_SLOTS_LOG2);
}
static inline size_t bit_reverse(size_t i, int bits)
{
    size_t j = 0;
    for (int b = 0; b < bits; b++) j |= ((i >> b) & 1) << (bits - 1 - b);
    return j;
}
// element i of t, i < 2 n: (c_(n-1), 0 x (n + 1), c_1 .. c_(n-2)) -> the index of the coefficient, or -1 for a zero
static inline long kzg_open_all_t_source(size_t i, size_t n)
{
    if (i == 0) return (long)(n - 1);
    if (i <= n + 1) return -1;
    return (long)(i - n - 1);
}

// S^ = DFT_N(s), s = (P_(n-2) .. P_0, infinity x (n + 1)), root W = fr_root_of_unity(log2n + 1); natural order.  Rows are the even entries of an endo
// table; one off the curve: BBGPU_ERR_ARG and its index in *bad_row.
static inline int kzg_open_all_setup_host(const uint64_t* table, size_t n, int log2n, std::vector<Xyzz>& S, uint64_t* bad_row)
{
    const size_t N = 2 * n;
    S.assign(N, g1_infinity());
    for (size_t j = 0; j + 1 < n; j++) {
        Fq px, py;
        g1_words_canonical(table + 16 * j, &px, &py);
        if (!g1_on_curve(px, py)) {
            *bad_row = j;
            return BBGPU_ERR_ARG;
        }
        S[bit_reverse(n - 2 - j, log2n + 1)] = Xyzz{ px, py, FQ_ONE, FQ_ONE };
    }
    g1_transform_host(S, log2n + 1, fr_root_of_unity(log2n + 1));
    return BBGPU_OK;
}

// the proofs of `batch` polynomials over S^: proofs_out[(b n + i) * 8] = the affine pi_b(omega^i), reference format (infinity: bit 63 of y[3], rest zero)
static inline void kzg_open_all_proofs_host(const std::vector<Xyzz>& S, size_t n, int log2n, const uint64_t* coeffs, size_t stride_elems, int batch,
                                            uint64_t* proofs_out)
{
    const size_t N = 2 * n;
    const int log2N = log2n + 1;
    const Fr W = fr_root_of_unity(log2N), Ninv = fr_inv(fr_from_u64((uint64_t)N));
    std::vector<uint64_t> t(4 * N);
    std::vector<Xyzz> v(N), u(n);
    for (int b = 0; b < batch; b++) {
        const uint64_t* c = coeffs + (size_t)b * stride_elems * 4;
        for (size_t i = 0; i < N; i++) {
            const long src = kzg_open_all_t_source(i, n);
            if (src < 0) memset(&t[4 * i], 0, 32);
            else memcpy(&t[4 * i], c + 4 * (size_t)src, 32);
        }
        ntt_radix2(t.data(), log2N, BBGPU_FFT, nullptr);
        fallback_parallel(N, 8, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                const size_t j = bit_reverse(i, log2N);
                Fr k;
                memcpy(k.d, &t[4 * j], 32);
                v[i] = g1_times_plain(S[j], fr_from_mont(fr_mul(k, Ninv)));
            }
        });
        g1_transform_host(v, log2N, fr_inv(W));
        for (size_t m = 0; m + 1 < n; m++) u[bit_reverse(m, log2n)] = v[m];
        u[n - 1] = g1_infinity(); // bit_reverse(n - 1) == n - 1
        g1_transform_host(u, log2n, fr_root_of_unity(log2n));
        uint64_t* out = proofs_out + (size_t)b * n * 8;
        fallback_parallel(n, 64, [&](size_t lo, size_t hi) {
            for (size_t i = lo; i < hi; i++) {
                uint64_t o[12];
                g1_to_normalised(u[i], o);
                memcpy(out + 8 * i, o, 64);
            }
        });
    }
}

} // namespace host
} // namespace bbgpu
