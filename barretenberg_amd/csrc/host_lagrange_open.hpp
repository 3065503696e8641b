// host_lagrange_open.hpp -- the host side of evaluation and opening in evaluation form (include/bbgpu.h, bbgpu_fr_evaluate_lagrange_device,
// bbgpu_kate_opening_lagrange_device): the argument verdict and the case decision the GPU entries and their host twins share (is z on the domain, and
// where), and the twins' own loops.  For a polynomial given by its values v_i = f(w^i) on the size-n domain and z outside it
//   f(z) = (z^n - 1) / n * sum_i v_i w^i / (z - w^i)            q_i = (f(z) - v_i) / (z - w^i)
// and for z = w^m:  f(z) = v_m,  q_i = (v_m - v_i) / (z - w^i) for i != m,  q_m = -sum_{i != m} q_i w^(i - m)  (the X^(n-1) coefficient of a quotient
// of degree n - 2 is zero).  No transform.  The twin is plain loops with Montgomery's trick for the n inversions -- deliberately NOT the launch
// structure of poly.hip; both sides write canonical field elements, so they agree bit for bit.  Product code, no oracle/; no HIP call, no lock.
// Behind them the fold sum_b gamma_b v_b and the opening of a fold (bbgpu_fr_fold_device, bbgpu_lagrange_opening_open_folded): the fold as a plain loop, then
// the definition above on the folded vector.  The sessions of the device side have no counterpart here: they are an economy, not part of the definition.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fr.hpp"

namespace bbgpu {
namespace host {

constexpr int LAGRANGE_OPEN_MAX_LOG2 = 24;
constexpr int LAGRANGE_OPEN_MAX_BATCH = 64;

// n = 2^k with 1 <= k <= 24 -> k, else -1
static inline int lagrange_open_log2(size_t n)
{
    for (int k = 1; k <= LAGRANGE_OPEN_MAX_LOG2; k++)
        if (n == (size_t)1 << k) return k;
    return -1;
}
// the size half of the argument verdict: n, batch, stride
static inline bool lagrange_open_sizes_ok(size_t n, size_t stride_elems, int batch)
{
    return lagrange_open_log2(n) >= 1 && batch >= 1 && batch <= LAGRANGE_OPEN_MAX_BATCH && stride_elems >= n;
}

// z (canonical) on the size-2^log2n domain?  z^n == 1 by log2 n squarings; then m with z = w^m bit by bit: with bits below b removed, the rest
// raised to 2^(log2n - 1 - b) is -1 exactly when bit b is set
static inline bool lagrange_open_on_domain(const Fr& z, int log2n, size_t* m_out)
{
    const Fr one = fr_one();
    Fr t = z;
    for (int i = 0; i < log2n; i++) t = fr_sqr(t);
    if (!fr_eq(t, one)) return false;
    Fr rest = z, wpow = fr_inv(fr_root_of_unity(log2n)); // w^-(2^b)
    size_t m = 0;
    for (int b = 0; b < log2n; b++) {
        t = rest;
        for (int i = 0; i < log2n - 1 - b; i++) t = fr_sqr(t);
        if (!fr_eq(t, one)) {
            m |= (size_t)1 << b;
            rest = fr_mul(rest, wpow);
        }
        wpow = fr_sqr(wpow);
    }
    *m_out = m;
    return true;
}
// (z^n - 1) / n: what the barycentric sum is multiplied by
static inline Fr lagrange_open_scale(const Fr& z, int log2n)
{
    Fr t = z;
    for (int i = 0; i < log2n; i++) t = fr_sqr(t);
    return fr_mul(fr_sub(t, fr_one()), fr_inv(fr_from_u64((uint64_t)1 << log2n)));
}

// values of polynomial b at values[(b * stride + i) * 4]; out (batch x 4, may be null) receives f_b(z); quotient (may be null: evaluation only, else
// the layout of values; may BE values) receives q_b.  Elements between the polynomials are neither read nor written.
static inline void lagrange_open_host(const uint64_t* values, uint64_t* quotient, size_t n, size_t stride, int batch, const Fr& z_any, uint64_t* out)
{
    const int log2n = lagrange_open_log2(n);
    const Fr one = fr_one(), z = fr_mul(z_any, one), w = fr_root_of_unity(log2n);
    size_t m = 0;
    const bool on = lagrange_open_on_domain(z, log2n, &m);
    // inv[i] = 1 / (z - w^i) (one at i == m), wi[i] = w^i: Montgomery's trick, one inversion for the whole batch
    std::vector<Fr> inv(n), wi(n), pre(n);
    Fr x = one, run = one;
    for (size_t i = 0; i < n; i++) {
        wi[i] = x;
        inv[i] = (on && i == m) ? one : fr_sub(z, x);
        pre[i] = run;
        run = fr_mul(run, inv[i]);
        x = fr_mul(x, w);
    }
    Fr r = fr_inv(run);
    for (size_t i = n; i-- > 0;) {
        const Fr d = inv[i];
        inv[i] = fr_mul(r, pre[i]);
        r = fr_mul(r, d);
    }
    const Fr scale = on ? fr_zero() : lagrange_open_scale(z, log2n);
    const Fr wm_inv = on ? fr_inv(wi[m]) : one;
    for (int b = 0; b < batch; b++) {
        const Fr* v = reinterpret_cast<const Fr*>(values) + (size_t)b * stride;
        Fr y;
        if (on) {
            y = fr_mul(v[m], one);
        } else {
            Fr acc = fr_zero();
            for (size_t i = 0; i < n; i++) acc = fr_add(acc, fr_mul(fr_mul(v[i], wi[i]), inv[i]));
            y = fr_mul(acc, scale);
        }
        if (out) memcpy(out + 4 * (size_t)b, y.d, 32);
        if (!quotient) continue;
        Fr* q = reinterpret_cast<Fr*>(quotient) + (size_t)b * stride;
        Fr acc = fr_zero();
        for (size_t i = 0; i < n; i++) {
            if (on && i == m) continue;
            q[i] = fr_mul(fr_sub(y, fr_mul(v[i], one)), inv[i]); // v[i] is read before q[i] is written: q may be v
            if (on) acc = fr_add(acc, fr_mul(fr_mul(q[i], wi[i]), wm_inv));
        }
        if (on) q[m] = fr_neg(acc);
    }
}

// ---- folds (bbgpu_fr_fold_device, bbgpu_lagrange_opening_open_folded and their twins) ------------------------------------------------------------------
constexpr size_t FOLD_MAX_N = (size_t)1 << 24;
// the fold alone takes any length, not only a domain's
static inline bool fold_sizes_ok(size_t n, size_t stride_elems, int batch)
{
    return n >= 1 && n <= FOLD_MAX_N && batch >= 1 && batch <= LAGRANGE_OPEN_MAX_BATCH && stride_elems >= n;
}
// out[i] = sum_b gamma_b v_{b,i}, or that added to out[i]; canonical.  out must not overlap values
static inline void fold_host(uint64_t* out, const uint64_t* values, size_t n, size_t stride, int batch, const uint64_t* gamma, bool accumulate)
{
    const Fr* v = reinterpret_cast<const Fr*>(values);
    const Fr* g = reinterpret_cast<const Fr*>(gamma);
    Fr* o = reinterpret_cast<Fr*>(out);
    const Fr one = fr_one();
    std::vector<Fr> gc((size_t)batch); // canonical: fr_mul takes one operand of any representative, not two
    for (int b = 0; b < batch; b++) gc[b] = fr_mul(g[b], one);
    for (size_t i = 0; i < n; i++) {
        Fr acc = accumulate ? fr_mul(o[i], one) : fr_zero();
        for (int b = 0; b < batch; b++) acc = fr_add(acc, fr_mul(v[(size_t)b * stride + i], gc[b]));
        o[i] = acc;
    }
}
// the opening of F = sum_b gamma_b f_b at z: quotient[i] = (or +=) the values of (F(X) - F(z)) / (X - z); f_out (may be null) = F(z).  Stateless: the fold,
// then the definition above on the folded vector
static inline void lagrange_open_folded_host(const uint64_t* values, size_t n, size_t stride, int batch, const uint64_t* gamma, const Fr& z, uint64_t* quotient,
                                             bool accumulate, uint64_t* f_out)
{
    std::vector<Fr> folded(n);
    fold_host(folded[0].d, values, n, stride, batch, gamma, false);
    if (!accumulate) {
        lagrange_open_host(folded[0].d, quotient, n, n, 1, z, f_out);
        return;
    }
    lagrange_open_host(folded[0].d, folded[0].d, n, n, 1, z, f_out);
    Fr* q = reinterpret_cast<Fr*>(quotient);
    for (size_t i = 0; i < n; i++) q[i] = fr_add(fr_mul(q[i], fr_one()), folded[i]);
}

} // namespace host
} // namespace bbgpu
