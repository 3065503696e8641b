// selftest_raw.hpp -- the raw-limb cases of bbgpu_selftest_field (BBGPU_SELFTEST_WIDE_*): one function per case, __host__ __device__, shared by the
// device self-test (selftest.hip) and the host twin the GPU test compares it with (tests/cpp/fe_wideq_twin.cpp).
#pragma once
#include "../../include/bbgpu.h"
#include "fe.hpp"

namespace bbgpu {

// ---- raw-limb ops: the wide quotient-digit forms themselves, limb for limb ------------------------------------------------------------------
// A case is THREE consecutive 32-byte rows of a, of b and of out, read as 24 words: a rows = the nine limbs of operand a, then of operand c;
// b rows = the nine limbs of operand b, then of operand d (a b + c d) or of the addend e (addhi forms); out rows = the nine limbs of the
// result, then zeros.  Limbs are taken as given (any 32-bit value: the caller keeps to what the form accepts).  __host__ __device__: the
// library runs it in a kernel, tests/cpp/fe_wideq_twin.cpp in a host loop, and the test compares the two outputs word for word.
template <class F> BB_HD void raw_case(int op, const uint32_t* ar, const uint32_t* br, uint32_t* o)
{
    uint32_t a[NL], b[NL], c[NL], d[NL], r[NL];
#pragma unroll
    for (int i = 0; i < NL; i++) {
        a[i] = ar[i];
        c[i] = ar[NL + i];
        b[i] = br[i];
        d[i] = br[NL + i];
        r[i] = 0;
    }
    switch (op) {
    case BBGPU_SELFTEST_WIDE_MUL: mul_raw<F, true>(a, b, r); break;
    case BBGPU_SELFTEST_WIDE_SQR: sqr_raw<F, true>(a, r); break;
    case BBGPU_SELFTEST_WIDE_MUL2: mul2_raw<F, true>(a, b, c, d, r); break;
    case BBGPU_SELFTEST_WIDE_MUL_IP:
        mul_raw_inplace<F, true>(a, b);
#pragma unroll
        for (int i = 0; i < NL; i++) r[i] = a[i];
        break;
    case BBGPU_SELFTEST_WIDE_MUL2_IP:
        mul2_raw_inplace<F, true>(a, b, c, d);
#pragma unroll
        for (int i = 0; i < NL; i++) r[i] = c[i];
        break;
    case BBGPU_SELFTEST_WIDE_MUL_ADDHI_IP:
        mul_addhi_raw_inplace<F, true>(a, b, d);
#pragma unroll
        for (int i = 0; i < NL; i++) r[i] = a[i];
        break;
    case BBGPU_SELFTEST_WIDE_SQR_ADDHI: sqr_addhi_raw<F, true>(a, d, r); break;
    default:
#pragma unroll
        for (int i = 0; i < NL; i++) r[i] = ~0u;
    }
#pragma unroll
    for (int i = 0; i < 24; i++) o[i] = i < NL ? r[i] : 0u;
}
// BBGPU_SELFTEST_WIDE_CHAIN: case i folds the operands a of cases i + 1, i + 2, ... (wrapping over the m cases), 255 of them, into operand a of case i,
// cycling through the four in-place shapes a loop-carried value takes: x <- x y, x <- x^2 + y, x <- y x + x y (one reduction), x <- x y + y.
// Operands are field values below 6 p with exact limbs; the carried value then stays below 9 p (x^2 / R + p + y < (81 / 169 + 7) p).
template <class F> BB_HD void raw_chain(const uint32_t* a_rows, int m, int i, uint32_t* o)
{
    uint32_t x[NL], y[NL], t[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) x[l] = a_rows[24 * (size_t)i + l];
    int at = i;
    for (int k = 0; k < 255; k++) {
        at = at + 1 == m ? 0 : at + 1;
#pragma unroll
        for (int l = 0; l < NL; l++) y[l] = a_rows[24 * (size_t)at + l];
        switch (k & 3) {
        case 0: mul_raw_inplace<F, true>(x, y); break;
        case 1:
            sqr_addhi_raw<F, true>(x, y, t);
#pragma unroll
            for (int l = 0; l < NL; l++) x[l] = t[l];
            break;
        case 2: mul2_raw_inplace<F, true>(y, x, x, y); break;
        default: mul_addhi_raw_inplace<F, true>(x, y, y); break;
        }
    }
#pragma unroll
    for (int l = 0; l < 24; l++) o[l] = l < NL ? x[l] : 0u;
}
template <class F> BB_HD void raw_dispatch(int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int m, int i)
{
    if (op == BBGPU_SELFTEST_WIDE_CHAIN) raw_chain<F>(a, m, i, out + 24 * (size_t)i);
    else raw_case<F>(op, a + 24 * (size_t)i, b + 24 * (size_t)i, out + 24 * (size_t)i);
}

} // namespace bbgpu
