// host_pairing.hpp -- the BN254 optimal-ate pairing on the host: the O(1) tail of the SRS check (two pairings for a table of any size) and the
// missing piece of a verifier.  Restates the algorithm of curves/bn254/pairing.cpp over the tower of fields/field{2,6,12}.hpp:
//   fq2 = fq[u] / (u^2 + 1)   fq6 = fq2[v] / (v^3 - xi), xi = 9 + u   fq12 = fq6[w] / (w^2 - v)
//   e(P, Q) = (f_{6z+2,Q}(P) * l_{[6z+2]Q, pi(Q)}(P) * l_{[6z+2]Q + pi(Q), -pi^2(Q)}(P)) ^ ((q^12 - 1) / r),   z = 4965661367192848881
// Miller loop over the signed digits of 6z + 2 with Q on the twist in homogeneous projective coordinates (doubling / mixed-addition steps that
// return the line's three fq2 coefficients: pairing.cpp:24-118), the line evaluated at P and multiplied in (:162-251), the two Frobenius additions
// (:13-22,149-159), then the final exponentiation: easy part f^((q^6 - 1)(q^2 + 1)) (:253-264), hard part by three powers of z (:266-331).
// Every constant the reference keeps as a table (the twist's b, the Frobenius coefficients, the digits of 6z + 2 and of z) is DERIVED here from
// q, xi and z on first use; the reduced pairing is a canonical value, so the 12 output coordinates equal the reference's bit for bit
// (tests/golden/pairing_kats.json).  Product code on host_g1.hpp / host_g2.hpp, no oracle/; no HIP call, no lock, re-entrant.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "host_fr.hpp"
#include "host_g1.hpp"
#include "host_g2.hpp"

namespace bbgpu {
namespace host {

static const uint64_t BN_Z = 4965661367192848881ULL; // the curve parameter: q and r are polynomials in it

// ---- fq2 beyond host_g2.hpp -------------------------------------------------------------------------------------------------------
static inline Fq fq_neg(const Fq& a) { return fq_sub(Fq{ { 0, 0, 0, 0 } }, a); }
static inline Fq fq_canonical(Fq a) // any 256-bit value: 2^256 < 6 q
{
    for (int i = 0; i < 5; i++) fq_cond_sub_p(a);
    return a;
}
static inline Fq2 fq2_zero() { return { { { 0, 0, 0, 0 } }, { { 0, 0, 0, 0 } } }; }
static inline Fq2 fq2_one() { return { FQ_ONE, { { 0, 0, 0, 0 } } }; }
static inline Fq2 fq2_neg(const Fq2& a) { return { fq_neg(a.c0), fq_neg(a.c1) }; }
static inline Fq2 fq2_conj(const Fq2& a) { return { a.c0, fq_neg(a.c1) }; } // the Frobenius of fq2
static inline Fq2 fq2_mul_fq(const Fq2& a, const Fq& k) { return { fq_mul(a.c0, k), fq_mul(a.c1, k) }; }
static inline bool fq2_eq(const Fq2& a, const Fq2& b) { return fq_eq(a.c0, b.c0) && fq_eq(a.c1, b.c1); }
static inline Fq2 fq2_mul_xi(const Fq2& a) // (9 + u)(a0 + a1 u) = (9 a0 - a1) + (9 a1 + a0) u
{
    const Fq a8 = fq_dbl(fq_dbl(fq_dbl(a.c0))), b8 = fq_dbl(fq_dbl(fq_dbl(a.c1)));
    return { fq_sub(fq_add(a8, a.c0), a.c1), fq_add(fq_add(b8, a.c1), a.c0) };
}
static inline Fq2 fq2_pow(const Fq2& a, const uint64_t e[4])
{
    Fq2 acc = fq2_one();
    for (int i = 255; i >= 0; --i) {
        acc = fq2_sqr(acc);
        if ((e[i >> 6] >> (i & 63)) & 1) acc = fq2_mul(acc, a);
    }
    return acc;
}

// ---- fq6 --------------------------------------------------------------------------------------------------------------------------
struct Fq6 {
    Fq2 c0, c1, c2;
};
static inline Fq6 fq6_zero() { return { fq2_zero(), fq2_zero(), fq2_zero() }; }
static inline Fq6 fq6_add(const Fq6& a, const Fq6& b) { return { fq2_add(a.c0, b.c0), fq2_add(a.c1, b.c1), fq2_add(a.c2, b.c2) }; }
static inline Fq6 fq6_sub(const Fq6& a, const Fq6& b) { return { fq2_sub(a.c0, b.c0), fq2_sub(a.c1, b.c1), fq2_sub(a.c2, b.c2) }; }
static inline Fq6 fq6_neg(const Fq6& a) { return { fq2_neg(a.c0), fq2_neg(a.c1), fq2_neg(a.c2) }; }
static inline Fq6 fq6_mul_v(const Fq6& a) { return { fq2_mul_xi(a.c2), a.c0, a.c1 }; } // v^3 = xi
static inline Fq6 fq6_mul_fq2(const Fq6& a, const Fq2& k) { return { fq2_mul(a.c0, k), fq2_mul(a.c1, k), fq2_mul(a.c2, k) }; }
static inline Fq6 fq6_mul(const Fq6& a, const Fq6& b) // six fq2 products (Karatsuba on the cross terms)
{
    const Fq2 t0 = fq2_mul(a.c0, b.c0), t1 = fq2_mul(a.c1, b.c1), t2 = fq2_mul(a.c2, b.c2);
    const Fq2 m12 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c1, a.c2), fq2_add(b.c1, b.c2)), t1), t2); // a1 b2 + a2 b1
    const Fq2 m01 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(b.c0, b.c1)), t0), t1); // a0 b1 + a1 b0
    const Fq2 m02 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c2), fq2_add(b.c0, b.c2)), t0), t2); // a0 b2 + a2 b0
    return { fq2_add(t0, fq2_mul_xi(m12)), fq2_add(m01, fq2_mul_xi(t2)), fq2_add(m02, t1) };
}
static inline Fq6 fq6_sqr(const Fq6& a) { return fq6_mul(a, a); }
static inline Fq6 fq6_inv(const Fq6& a) // the adjugate over the norm to fq2
{
    const Fq2 A = fq2_sub(fq2_sqr(a.c0), fq2_mul_xi(fq2_mul(a.c1, a.c2)));
    const Fq2 B = fq2_sub(fq2_mul_xi(fq2_sqr(a.c2)), fq2_mul(a.c0, a.c1));
    const Fq2 C = fq2_sub(fq2_sqr(a.c1), fq2_mul(a.c0, a.c2));
    const Fq2 norm = fq2_add(fq2_mul(a.c0, A), fq2_mul_xi(fq2_add(fq2_mul(a.c2, B), fq2_mul(a.c1, C))));
    const Fq2 ni = fq2_inv(norm);
    return { fq2_mul(A, ni), fq2_mul(B, ni), fq2_mul(C, ni) };
}

// ---- fq12 -------------------------------------------------------------------------------------------------------------------------
struct Fq12 {
    Fq6 c0, c1;
};
static inline Fq12 fq12_one() { return { { fq2_one(), fq2_zero(), fq2_zero() }, fq6_zero() }; }
static inline bool fq12_eq(const Fq12& a, const Fq12& b) { return !memcmp(&a, &b, sizeof(Fq12)); } // canonical coordinates, no padding: 12 x 32 bytes
static inline Fq12 fq12_mul(const Fq12& a, const Fq12& b)
{
    const Fq6 t0 = fq6_mul(a.c0, b.c0), t1 = fq6_mul(a.c1, b.c1);
    const Fq6 cross = fq6_sub(fq6_sub(fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1)), t0), t1);
    return { fq6_add(t0, fq6_mul_v(t1)), cross }; // w^2 = v
}
static inline Fq12 fq12_sqr(const Fq12& a) // (a0 + a1)(a0 + v a1) - t - v t = a0^2 + v a1^2,  t = a0 a1
{
    const Fq6 t = fq6_mul(a.c0, a.c1);
    const Fq6 s = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(a.c0, fq6_mul_v(a.c1)));
    return { fq6_sub(fq6_sub(s, t), fq6_mul_v(t)), fq6_add(t, t) };
}
static inline Fq12 fq12_conj(const Fq12& a) { return { a.c0, fq6_neg(a.c1) }; } // = a^(q^6); the inverse of a unitary element
static inline Fq12 fq12_inv(const Fq12& a)
{
    const Fq6 ni = fq6_inv(fq6_sub(fq6_sqr(a.c0), fq6_mul_v(fq6_sqr(a.c1))));
    return { fq6_mul(a.c0, ni), fq6_neg(fq6_mul(a.c1, ni)) };
}

// ---- constants derived from q, xi, z ------------------------------------------------------------------------------------------------
struct PairingConsts {
    Fq two_inv;
    Fq2 twist_b;     // 3 / xi: the twist is y^2 = x^3 + 3 / xi
    Fq2 gamma[3][5]; // gamma[k - 1][j - 1] = xi^(j (q^k - 1) / 6): w^j -> gamma w^j under the k-th power of the Frobenius
    int8_t loop_digit[68]; // signed digits (non-adjacent form) of 6z + 2, least significant first; loop_top indexes the top one
    int loop_top;
    PairingConsts()
    {
        two_inv = fq_inv(fq_dbl(FQ_ONE));
        const Fq three = fq_add(fq_dbl(FQ_ONE), FQ_ONE);
        const Fq nine = fq_add(fq_dbl(fq_dbl(fq_dbl(FQ_ONE))), FQ_ONE);
        const Fq2 xi = { nine, FQ_ONE };
        twist_b = fq2_mul_fq(fq2_inv(xi), three);
        uint64_t e[4]; // (q - 1) / 6
        u128 rem = 0;
        for (int i = 3; i >= 0; --i) {
            const u128 cur = (rem << 64) | (i == 0 ? FQ_P[0] - 1 : FQ_P[i]);
            e[i] = (uint64_t)(cur / 6);
            rem = cur % 6;
        }
        const Fq2 g1 = fq2_pow(xi, e);
        // x^q = conj(x) in fq2, so xi^((q^2 - 1) / 6) = g1^(q + 1) = conj(g1) g1 and xi^((q^3 - 1) / 6) = g1^(q^2 + q + 1) = g1 conj(g1) g1
        const Fq2 g2 = fq2_mul(fq2_conj(g1), g1), g3 = fq2_mul(g2, g1);
        const Fq2 base[3] = { g1, g2, g3 };
        for (int k = 0; k < 3; k++) {
            gamma[k][0] = base[k];
            for (int j = 1; j < 5; j++) gamma[k][j] = fq2_mul(gamma[k][j - 1], base[k]);
        }
        u128 s = (u128)BN_Z * 6 + 2;
        loop_top = 0;
        memset(loop_digit, 0, sizeof loop_digit);
        for (int i = 0; s; i++) {
            int d = 0;
            if (s & 1) {
                d = (s & 3) == 3 ? -1 : 1;
                if (d < 0) s += 1;
                else s -= 1;
            }
            loop_digit[i] = (int8_t)d;
            if (d) loop_top = i;
            s >>= 1;
        }
    }
};
static inline const PairingConsts& pairing_consts()
{
    static const PairingConsts c; // initialised once, thread-safe
    return c;
}

// a^(q^k), k = 1, 2, 3: the coordinate of w^j (j = 0 .. 5; w^2 = v) is conjugated for odd k and multiplied by gamma[k - 1][j - 1]
static inline Fq12 fq12_frobenius(const Fq12& a, int k)
{
    const PairingConsts& K = pairing_consts();
    auto co = [&](const Fq2& x, int j) {
        const Fq2 t = (k & 1) ? fq2_conj(x) : x;
        return j ? fq2_mul(t, K.gamma[k - 1][j - 1]) : t;
    };
    // c0 = (1, v, v^2) = (w^0, w^2, w^4), c1 = (w, w^3, w^5)
    return { { co(a.c0.c0, 0), co(a.c0.c1, 2), co(a.c0.c2, 4) }, { co(a.c1.c0, 1), co(a.c1.c1, 3), co(a.c1.c2, 5) } };
}

// ---- Miller loop ---------------------------------------------------------------------------------------------------------------------
struct G2Proj {
    Fq2 x, y, z; // homogeneous: (x / z, y / z)
};
struct Line { // the line through the step's points at a G1 argument (px, py): o + (vw py) v w + (vv px) v^2
    Fq2 o, vw, vv;
};
// T <- 2 T and the tangent at T   (pairing.cpp:24-77)
static inline Line miller_double(G2Proj& T)
{
    const PairingConsts& K = pairing_consts();
    const Fq2 A = fq2_mul(fq2_mul_fq(T.x, K.two_inv), T.y); // x y / 2
    const Fq2 B = fq2_sqr(T.y), C = fq2_sqr(T.z);
    const Fq2 E = fq2_mul(K.twist_b, fq2_add(fq2_dbl(C), C)); // 3 b' z^2
    const Fq2 F = fq2_add(fq2_dbl(E), E);
    const Fq2 G = fq2_mul_fq(fq2_add(B, F), K.two_inv);
    const Fq2 H = fq2_sub(fq2_sqr(fq2_add(T.y, T.z)), fq2_add(B, C)); // 2 y z
    const Fq2 I = fq2_sub(E, B), J = fq2_sqr(T.x), EE = fq2_sqr(E);
    T.x = fq2_mul(A, fq2_sub(B, F));
    T.y = fq2_sub(fq2_sqr(G), fq2_add(fq2_dbl(EE), EE));
    T.z = fq2_mul(B, H);
    return { fq2_mul_xi(I), fq2_neg(H), fq2_add(fq2_dbl(J), J) };
}
// T <- T + (bx, by) and the line through both   (pairing.cpp:79-118)
static inline Line miller_add(G2Proj& T, const Fq2& bx, const Fq2& by)
{
    const Fq2 D = fq2_sub(T.x, fq2_mul(bx, T.z)), E = fq2_sub(T.y, fq2_mul(by, T.z));
    const Fq2 F = fq2_sqr(D), G = fq2_sqr(E), H = fq2_mul(D, F), I = fq2_mul(T.x, F);
    const Fq2 J = fq2_sub(fq2_add(fq2_mul(T.z, G), H), fq2_dbl(I));
    const Fq2 y3 = fq2_sub(fq2_mul(fq2_sub(I, J), E), fq2_mul(T.y, H));
    T.x = fq2_mul(D, J);
    T.y = y3;
    T.z = fq2_mul(T.z, H);
    return { fq2_mul_xi(fq2_sub(fq2_mul(E, bx), fq2_mul(D, by))), D, fq2_neg(E) };
}
// f <- f * line(P): the line is sparse in fq12 -- c0 = (o, 0, vv px), c1 = (0, vw py, 0) (field12.hpp:79-148)
static inline Fq12 fq12_mul_line(const Fq12& f, const Line& l, const Fq& px, const Fq& py)
{
    const Fq12 s = { { l.o, fq2_zero(), fq2_mul_fq(l.vv, px) }, { fq2_zero(), fq2_mul_fq(l.vw, py), fq2_zero() } };
    return fq12_mul(f, s);
}

struct PairingInput {
    Fq px, py;
    G2Affine q;
};
// prod_k f_{6z+2, Q_k}(P_k) with the two Frobenius lines: ONE squaring per loop digit for all pairs (pairing.cpp:202-251)
static inline Fq12 miller_loop(const PairingInput* in, size_t count)
{
    const PairingConsts& K = pairing_consts();
    std::vector<G2Proj> T(count);
    for (size_t k = 0; k < count; k++) T[k] = { in[k].q.x, in[k].q.y, fq2_one() };
    Fq12 f = fq12_one();
    for (int i = K.loop_top - 1; i >= 0; --i) {
        f = fq12_sqr(f);
        for (size_t k = 0; k < count; k++) f = fq12_mul_line(f, miller_double(T[k]), in[k].px, in[k].py);
        const int d = K.loop_digit[i];
        if (d == 0) continue;
        for (size_t k = 0; k < count; k++)
            f = fq12_mul_line(f, miller_add(T[k], in[k].q.x, d > 0 ? in[k].q.y : fq2_neg(in[k].q.y)), in[k].px, in[k].py);
    }
    // pi(Q) = (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2)) on the twist; the second point is -pi^2(Q)
    for (size_t k = 0; k < count; k++) {
        const Fq2 x1 = fq2_mul(fq2_conj(in[k].q.x), K.gamma[0][1]), y1 = fq2_mul(fq2_conj(in[k].q.y), K.gamma[0][2]);
        const Fq2 x2 = fq2_mul(fq2_conj(x1), K.gamma[0][1]), y2 = fq2_mul(fq2_conj(y1), K.gamma[0][2]);
        f = fq12_mul_line(f, miller_add(T[k], x1, y1), in[k].px, in[k].py);
        f = fq12_mul_line(f, miller_add(T[k], x2, fq2_neg(y2)), in[k].px, in[k].py);
    }
    return f;
}

// ---- final exponentiation --------------------------------------------------------------------------------------------------------------
static inline Fq12 fq12_pow_neg_z(const Fq12& a) // a^(-z) for a unitary a   (pairing.cpp:266-281)
{
    Fq12 r = a;
    for (int i = 61; i >= 0; --i) { // z has 63 bits
        r = fq12_sqr(r);
        if ((BN_Z >> i) & 1) r = fq12_mul(r, a);
    }
    return fq12_conj(r);
}
static inline Fq12 final_exponentiation(const Fq12& f)
{
    // easy part: f^(q^6 - 1) = conj(f) / f, then the (q^2 + 1)-th power; the result is unitary (its inverse is its conjugate)
    Fq12 e = fq12_mul(fq12_conj(f), fq12_inv(f));
    e = fq12_mul(fq12_frobenius(e, 2), e);
    // hard part, (q^4 - q^2 + 1) / r, from e^(-z), e^(z^2), e^(-z^3) and the Frobenius maps (pairing.cpp:283-331)
    const Fq12 A = fq12_pow_neg_z(e), B = fq12_sqr(A), C = fq12_sqr(B), D = fq12_mul(C, B);
    const Fq12 E = fq12_pow_neg_z(D), F = fq12_sqr(E), G = fq12_pow_neg_z(F);
    const Fq12 K = fq12_mul(fq12_conj(D), fq12_mul(fq12_conj(G), E));
    const Fq12 L = fq12_mul(B, K), N = fq12_mul(fq12_mul(E, K), e);
    const Fq12 R = fq12_mul(fq12_mul(fq12_frobenius(L, 1), N), fq12_frobenius(K, 2));
    return fq12_mul(R, fq12_frobenius(fq12_mul(L, fq12_conj(e)), 3));
}

// ---- the reference's memory formats ---------------------------------------------------------------------------------------------------
static inline bool g1_words_is_inf(const uint64_t p[8]) { return (p[7] >> 63) & 1; }
static inline G2Affine g2_from_words(const uint64_t q[16])
{
    G2Affine r;
    memcpy(&r, q, 128);
    r.x.c0 = fq_canonical(r.x.c0);
    r.x.c1 = fq_canonical(r.x.c1);
    r.y.c0 = fq_canonical(r.y.c0);
    r.y.c1 = fq_canonical(r.y.c1);
    return r;
}
// prod_k e(P_k, Q_k) with one shared final exponentiation (reduced_ate_pairing_batch, pairing.cpp:364-385); a pair whose P is the point at infinity
// contributes one.  p: count x 8 words, q: count x 16 words.
static inline Fq12 pairing_product(const uint64_t* p, const uint64_t* q, size_t count)
{
    std::vector<PairingInput> in;
    in.reserve(count);
    for (size_t k = 0; k < count; k++) {
        if (g1_words_is_inf(p + 8 * k)) continue;
        PairingInput e;
        memcpy(e.px.d, p + 8 * k, 32);
        memcpy(e.py.d, p + 8 * k + 4, 32);
        e.px = fq_canonical(e.px);
        e.py = fq_canonical(e.py);
        e.q = g2_from_words(q + 16 * k);
        in.push_back(e);
    }
    if (in.empty()) return fq12_one();
    return final_exponentiation(miller_loop(in.data(), in.size()));
}

// is q a usable x * G2: on the twist curve y^2 = x^3 + 3 / xi and of order r (the twist's group is larger than G2: cofactor 2q - r)
static inline bool g2_on_curve(const G2Affine& q)
{
    const Fq2 rhs = fq2_add(fq2_mul(fq2_sqr(q.x), q.x), pairing_consts().twist_b);
    return fq2_eq(fq2_sqr(q.y), rhs);
}
static inline bool g2_has_order_r(const G2Affine& q)
{
    G2Jac acc = { q.x, q.y, fq2_zero() };
    for (int i = 255; i >= 0; --i) {
        acc = g2_dbl(acc);
        if ((FrHostP::P[i >> 6] >> (i & 63)) & 1) acc = g2_madd(acc, q);
    }
    return fq2_is_zero(acc.z);
}

} // namespace host
} // namespace bbgpu
