// host_kzg_check_cells.hpp -- the check of KZG CELL proofs by ONE pairing product (include/bbgpu.h: bbgpu_kzg_check_cells, bbgpu_kzg_check_open_cosets, the
// _layout entries of up to 2^16 commitments, the host twins of all four and bbgpu_host_kzg_cells_key_check): the forms a call takes, the argument verdicts, the twins' own loops.  The findings, the report and the
// pairing tail with its bisection are host_kzg_check_batch.hpp's, with [x^l] G2 in the pairing.  Notation: l = coset, m = n / l, omega the root of the
// size-n domain, psi = omega^l, zeta = omega^m.  Cell k of f holds v_j = f(omega^(k + m j)), j < l; its proof pi_k has f = q_k (X^l - psi^k) + r_k with
//   r_k = sum_i a_i X^i,   a_i = omega^(-k i) l^-1 sum_j v_j zeta^(-i j)          (a size-l inverse transform, then a twist)
// and the cells t < count (label c_t, cell k_t, multipliers rho_t of bbgpu_srs_check) hold when e(A, G2) e(-B, [x^l] G2) == 1 for
//   A = sum_c (sum_{t: c_t = c} rho_t) C_c - sum_{i < l} (sum_t rho_t a_{t,i}) P_i + sum_t (rho_t psi^(k_t)) pi_t,   B = sum_t rho_t pi_t
// P_0 .. P_(l-1) the first l rows of the monomial string.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_kzg_check_batch.hpp"

namespace bbgpu {
namespace host {

constexpr size_t KZG_CELLS_MAX_N = (size_t)1 << 21;

// One call in either form.  Labelled: cell t is cell cell[t] of commitments[which[t]], its values at values[(t l + j) * 4].  Open-cosets: cell t = b m + k
// is cell k of commitment b, its values the entries k, k + m, .. of the transform at values[b * stride * 4].
struct KzgCellsCall {
    const uint64_t* commitments = nullptr;
    size_t S = 0;
    const uint32_t* which = nullptr; // labelled form
    const uint32_t* cell = nullptr;  // labelled form
    const uint64_t* values = nullptr;
    const uint64_t* proofs = nullptr;
    const uint64_t* head = nullptr;  // P_0 .. P_(l-1)
    size_t count = 0;
    int log2n = 0, log2l = 0;
    bool cosets = false;
    size_t stride = 0; // open-cosets form: elements between the transforms

    size_t l() const { return (size_t)1 << log2l; }
    size_t m() const { return (size_t)1 << (log2n - log2l); }
    size_t rows_head() const { return S + l(); } // rows of A before the cells' own: the shared commitments, then P_0 .. P_(l-1)
    size_t label(size_t t) const { return cosets ? t >> (log2n - log2l) : which[t]; }
    size_t cell_of(size_t t) const { return cosets ? t & (m() - 1) : cell[t]; }
    const uint64_t* value(size_t t, size_t j) const
    {
        return cosets ? values + (label(t) * stride + cell_of(t) + m() * j) * 4 : values + (t * l() + j) * 4;
    }
};

static inline int kzg_cells_log2(size_t v)
{
    int lg = 0;
    while (((size_t)1 << lg) < v) lg++;
    return lg;
}
// the sizes both forms share: coset and n powers of two, 1 <= coset <= 64, n / coset >= 2, n <= 2^21
static inline bool kzg_cells_domain_ok(size_t n, size_t coset, int* log2n, int* log2l)
{
    if (coset < 1 || coset > BBGPU_KZG_OPEN_COSETS_MAX_COSET || (coset & (coset - 1)) || n < 1 || (n & (n - 1)) || n > KZG_CELLS_MAX_N || n / coset < 2)
        return false;
    *log2n = kzg_cells_log2(n);
    *log2l = kzg_cells_log2(coset);
    return true;
}

// The argument verdicts every entry gives before anything else, sizes first: 0, or the code with `why` written.  K is filled in by the caller except
// log2n / log2l; batch is read in the open-cosets form only.  max_commitments: 64, or 2^16 for the layout entries -- the one thing they change here.
static inline int kzg_cells_args(KzgCellsCall* K, size_t n, size_t coset, int batch, const uint64_t* g2_xl, int flags, const bbgpu_kzg_check_report* out,
                                 char* why, size_t cap, size_t max_commitments = BBGPU_KZG_CHECK_MAX_COMMITMENTS)
{
    if (!kzg_cells_domain_ok(n, coset, &K->log2n, &K->log2l)) {
        snprintf(why, cap, "coset a power of two in 1 .. 64, n a power of two with 2 coset <= n <= 2^21 are taken");
        return BBGPU_ERR_SIZE;
    }
    if (K->cosets) {
        if (batch < 1 || (size_t)batch > max_commitments || K->stride < n || (size_t)batch * n > BBGPU_KZG_CHECK_MAX_CLAIMS) {
            snprintf(why, cap, "1 <= batch <= %zu, stride >= n and batch x n <= 2^20 are taken", max_commitments);
            return BBGPU_ERR_SIZE;
        }
        K->S = (size_t)batch;
        K->count = (size_t)batch * K->m();
    }
    if (K->count < 1 || K->count > BBGPU_KZG_CHECK_MAX_CLAIMS || K->count * coset > BBGPU_KZG_CHECK_MAX_CLAIMS) {
        snprintf(why, cap, "1 .. 2^20 cells of at most 2^20 values together are taken");
        return BBGPU_ERR_SIZE;
    }
    if (!K->commitments || !K->values || !K->proofs || !K->head || !g2_xl || !out || (!K->cosets && (!K->which || !K->cell))) {
        snprintf(why, cap, "null commitments / which / cell / values / proofs / g1_head / g2_xl / report");
        return BBGPU_ERR_ARG;
    }
    if (flags & ~BBGPU_KZG_CHECK_LOCATE) {
        snprintf(why, cap, "unknown flag bits");
        return BBGPU_ERR_ARG;
    }
    if (!K->cosets) {
        if (K->S < 1 || K->S > max_commitments) {
            snprintf(why, cap, "1 .. %zu shared commitments are taken", max_commitments);
            return BBGPU_ERR_ARG;
        }
        for (size_t t = 0; t < K->count; t++)
            if (K->which[t] >= K->S || K->cell[t] >= K->m()) {
                snprintf(why, cap, "cell %zu: %s", t, K->which[t] >= K->S ? "its label names no commitment" : "its cell index is not below n / coset");
                return BBGPU_ERR_ARG;
            }
    }
    if (!srs_check_g2_ok(g2_xl)) {
        snprintf(why, cap, "g2_xl is at infinity, off the twist curve or not of order r");
        return BBGPU_ERR_ARG;
    }
    for (size_t i = 0; i < coset; i++)
        if (g1_words_is_inf(K->head + 8 * i) || !g1_words_on_curve(K->head + 8 * i)) { // a key, not a claim
            snprintf(why, cap, "g1_head row %zu is %s", i, g1_words_is_inf(K->head + 8 * i) ? "at infinity" : "off the curve");
            return BBGPU_ERR_ARG;
        }
    return BBGPU_OK;
}

// bbgpu_host_kzg_cells_key_check behind its null checks: g2_xl usable and e(P_(l-1), x G2) e(-G, [x^l] G2) == 1
static inline bool kzg_cells_key_ok(const uint64_t* g1_head, size_t coset, const uint64_t g2_x[16], const uint64_t g2_xl[16])
{
    const uint64_t* last = g1_head + 8 * (coset - 1);
    if (!srs_check_g2_ok(g2_xl) || !srs_check_g2_ok(g2_x) || g1_words_is_inf(last) || !g1_words_on_curve(last)) return false;
    uint64_t top[8], gen[8];
    verify_own_point(last, top);
    g1_generator_words(gen);
    return pair_is_one(top, gen, g2_x, g2_xl);
}

// what the twin and the GPU driver both need of the domain: zeta^-e for e < l, omega^-1, psi, l^-1
struct KzgCellsDomain {
    std::vector<Fr> zeta_inv; // zeta^(-e), e < l
    Fr omega_inv, psi, l_inv;
};
static inline KzgCellsDomain kzg_cells_domain(int log2n, int log2l)
{
    KzgCellsDomain D;
    const size_t l = (size_t)1 << log2l;
    const Fr omega = fr_root_of_unity(log2n);
    D.omega_inv = fr_inv(omega);
    D.psi = fr_pow(omega, l);
    D.l_inv = fr_inv(fr_from_u64(l));
    const Fr zi = fr_pow(D.omega_inv, (uint64_t)1 << (log2n - log2l));
    D.zeta_inv.resize(l);
    Fr p = fr_one();
    for (size_t e = 0; e < l; e++) {
        D.zeta_inv[e] = p;
        p = fr_mul(p, zi);
    }
    return D;
}

// a_0 .. a_(l-1) of cell t: the decimation-in-frequency inverse transform in place (outputs in bit-reversed order), then the twist
static inline void kzg_cell_coefficients(const KzgCellsCall& K, const KzgCellsDomain& D, size_t t, Fr* a)
{
    const size_t l = K.l();
    std::vector<Fr> x(l);
    for (size_t j = 0; j < l; j++) {
        memcpy(x[j].d, K.value(t, j), 32);
        x[j] = fr_mul(x[j], fr_one()); // any representative below 2^256 -> canonical
    }
    for (size_t h = l / 2; h >= 1; h >>= 1)
        for (size_t b = 0; b < l; b += 2 * h)
            for (size_t q = 0; q < h; q++) {
                const Fr u = x[b + q], v = x[b + q + h];
                x[b + q] = fr_add(u, v);
                x[b + q + h] = fr_mul(fr_sub(u, v), D.zeta_inv[q * (l / (2 * h))]);
            }
    const Fr step = fr_pow(D.omega_inv, K.cell_of(t)); // omega^(-k)
    Fr tw = D.l_inv;
    for (size_t i = 0; i < l; i++) {
        size_t rev = 0;
        for (int b = 0; b < K.log2l; b++) rev |= ((i >> b) & 1) << (K.log2l - 1 - b);
        a[i] = fr_mul(x[rev], tw);
        tw = fr_mul(tw, step);
    }
}

// Both twins behind their argument checks; seed: the one in use.  Rows as the GPU driver lays them out: the S commitments, P_0 .. P_(l-1), then pi_t, so
// that a prefix of the cells is a prefix of both tables; B reads the same rows from the first cell on.
static inline int kzg_cells_host(const KzgCellsCall& K, const uint64_t g2_xl[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* R)
{
    kzg_report_init(R, K.count, seed);
    const size_t S = K.S, l = K.l(), H = K.rows_head(), count = K.count;
    uint64_t shared_bad = 0, shared_first = UINT64_MAX, claims_bad = 0, claims_key = UINT64_MAX;
    for (size_t c = 0; c < S; c++)
        if (!g1_words_acceptable(K.commitments + 8 * c) && shared_bad++ == 0) shared_first = c;
    for (size_t t = 0; t < count; t++)
        if (!g1_words_acceptable(K.proofs + 8 * t) && claims_bad++ == 0) claims_key = 2 * t + 1;
    kzg_report_findings(R, shared_bad, shared_first, claims_bad, claims_key);
    if (R->bad_points) return BBGPU_OK;

    std::vector<uint64_t> pts((H + count) * 8), sc_a((H + count) * 4, 0), sc_b(count * 4, 0);
    std::vector<Fr> rho(count), term(count * l);
    std::vector<bool> shared_inf(S);
    for (size_t c = 0; c < S; c++) shared_inf[c] = kzg_row(K.commitments + 8 * c, &pts[8 * c]);
    for (size_t i = 0; i < l; i++) (void)kzg_row(K.head + 8 * i, &pts[8 * (S + i)]);
    const KzgCellsDomain D = kzg_cells_domain(K.log2n, K.log2l);
    fallback_parallel(count, 64, [&](size_t lo, size_t hi) {
        std::vector<Fr> a(l);
        for (size_t t = lo; t < hi; t++) {
            srs_check_rho(seed, t, rho[t].d);
            kzg_cell_coefficients(K, D, t, a.data());
            for (size_t i = 0; i < l; i++) term[t * l + i] = fr_mul(a[i], rho[t]);
            if (!kzg_row(K.proofs + 8 * t, &pts[8 * (H + t)])) {
                const Fr rz = fr_mul(fr_pow(D.psi, K.cell_of(t)), rho[t]);
                memcpy(&sc_a[4 * (H + t)], rz.d, 32);
                memcpy(&sc_b[4 * t], rho[t].d, 32);
            }
        }
    });
    return kzg_check_tail(R, g2_xl, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) {
        std::vector<Fr> acc(H, fr_zero());
        for (size_t t = 0; t < m; t++) {
            acc[K.label(t)] = fr_add(acc[K.label(t)], rho[t]);
            for (size_t i = 0; i < l; i++) acc[S + i] = fr_add(acc[S + i], term[t * l + i]);
        }
        for (size_t i = 0; i < l; i++) acc[S + i] = fr_neg(acc[S + i]); // zero stays zero
        for (size_t c = 0; c < S; c++)
            if (shared_inf[c]) acc[c] = fr_zero(); // a stand-in row
        memcpy(sc_a.data(), acc.data(), H * 32);
        g1_to_normalised(msm_pippenger(sc_a.data(), pts.data(), H + m, 8), a12);
        g1_to_normalised(msm_pippenger(sc_b.data(), pts.data() + 8 * H, m, 8), b12);
        return (int)BBGPU_OK;
    });
}

} // namespace host
} // namespace bbgpu
