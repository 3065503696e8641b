// g1_ladder.hpp -- k * P for one point per lane, the body of k_srs_update (srs_update.hip) and of the butterflies of srs_lagrange.hip: the endomorphism split
// of the scalar in 64-bit integer C++, the group law on points whose bounds say what the formulas deliver, and ONE ladder over both halves of the split with
// fixed windows of odd signed digits.  The base may be projective (XYZZ) and the result stays projective (ladder_pt); ladder_row is the affine-in, affine-out
// form with the Fermat inversion behind it.  __host__ __device__ like the field code under it, so that the same code runs on the CPU against the host group law
// (tests/cpp).  The reference has the pieces only: the split (fields/field.hpp:413-485, restated for the host in host_wnaf.hpp) and the windows
// (groups/wnaf.hpp:15-55).
#pragma once
#include <type_traits>

#include "g1.hpp"

namespace bbgpu {

// ---- the endomorphism split in 64-bit integer C++ ------------------------------------------------------------------------------------------------------
// host_wnaf.hpp split_endo restated (constants field.hpp:420-426): c1 = (g2 k) >> 256, c2 = (g1 k) >> 256, t = c2 b2 - c1 (-b1), k2 = t, k1 = k + t lambda.
// One difference: t is taken as a SIGNED integer.  The floors make t = (-b1) frac(g2 k / 2^256) - b2 frac(g1 k / 2^256) up to the truncation of g1, g2: for
// k just above a multiple of 2^256 / g2 (k = ceil(2^256 / g2) is one) it is negative, and the host routine -- like the reference -- then returns the low
// limbs of r - |t|, which is not a split of k.  Here |k1|, |k2| < 2^128 always and the signs are applied to the points; where t >= 0 and k1 >= 0 the
// magnitudes are split_endo's values limb for limb (tests/golden/endo_wnaf.json through bbgpu_selftest_endo_split).
BB_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
template <int NA, int NB> BB_HD void mul_limbs(const uint64_t (&a)[NA], const uint64_t (&b)[NB], uint64_t (&r)[NA + NB])
{
#pragma unroll
    for (int i = 0; i < NA + NB; i++) r[i] = 0;
#pragma unroll
    for (int i = 0; i < NA; i++) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const uint64_t lo = a[i] * b[j], hi = mulhi64(a[i], b[j]);
            const uint64_t s = r[i + j] + lo, s2 = s + carry;
            carry = hi + (uint64_t)(s < lo) + (uint64_t)(s2 < carry); // a b + r + carry < 2^128: no overflow
            r[i + j] = s2;
        }
        r[i + NB] = carry;
    }
}
BB_HD uint64_t sub256(const uint64_t (&a)[4], const uint64_t (&b)[4], uint64_t (&r)[4]) // r = a - b mod 2^256, returns the borrow
{
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t d = a[i] - b[i], d2 = d - borrow;
        borrow = (uint64_t)(a[i] < b[i]) | (uint64_t)(d < borrow);
        r[i] = d2;
    }
    return borrow;
}
BB_HD void add256(const uint64_t (&a)[4], const uint64_t (&b)[4], uint64_t (&r)[4])
{
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t s = a[i] + b[i], s2 = s + carry;
        carry = (uint64_t)(s < b[i]) | (uint64_t)(s2 < carry);
        r[i] = s2;
    }
}
BB_HD void cond_sub_r(uint64_t (&a)[4]) // a -= r if a >= r
{
    const uint64_t r[4] = { FrP::P64[0], FrP::P64[1], FrP::P64[2], FrP::P64[3] };
    uint64_t d[4];
    const uint64_t borrow = sub256(a, r, d);
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = borrow ? a[i] : d[i];
}
struct EndoK {
    static constexpr uint32_t LAMBDA_M261[9] = { 0x1065364du, 0x19a50e73u, 0x5348a9cu, 0x2af1c94u, 0x11265ae2u, 0xa454b5au, 0x6633a88u, 0x1dbec294u, 0x38f7u }; // lambda 2^261 mod r (fr.hpp:54-57 re-limbed)
};
struct EndoSplit {
    uint64_t k1[2], k2[2]; // magnitudes
    bool neg1, neg2;       // k = (neg1 ? -k1 : k1) - lambda (neg2 ? -k2 : k2)  (mod r)
    bool fits;             // both magnitudes below 2^128 (always; reported by the self-test)
};
BB_HD void endo_split(const uint64_t (&k)[4], EndoSplit& s)
{
    const uint64_t G1[3] = { 0x7a7bd9d4391eb18dULL, 0x4ccef014a773d2cfULL, 0x2ULL };
    const uint64_t G2[2] = { 0xd91d232ec7e0b3d7ULL, 0x2ULL };
    const uint64_t MINUS_B1[2] = { 0x8211bbeb7d4f1128ULL, 0x6f4d8248eeb859fcULL };
    const uint64_t B2[1] = { 0x89d3256894d213e3ULL };
    uint64_t p1[6], p2[7];
    mul_limbs<2, 4>(G2, k, p1);
    mul_limbs<3, 4>(G1, k, p2);
    const uint64_t c1[2] = { p1[4], p1[5] }, c2[3] = { p2[4], p2[5], p2[6] };
    uint64_t q1[4], q2[4], t[4];
    mul_limbs<2, 2>(c1, MINUS_B1, q1); // < 2^66 2^127
    mul_limbs<3, 1>(c2, B2, q2);       // < 2^130 2^64
    s.neg2 = sub256(q2, q1, t) != 0;
    if (s.neg2) {
        const uint64_t zero[4] = { 0, 0, 0, 0 }, v[4] = { t[0], t[1], t[2], t[3] };
        (void)sub256(zero, v, t);
    }
    // lambda |t| mod r: lambda is held in Montgomery form, so the Montgomery product with the plain |t| is the plain product
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w[2 * i] = (uint32_t)t[i];
        w[2 * i + 1] = (uint32_t)(t[i] >> 32);
    }
    uint32_t mw[8];
    to_canonical(mul(unpack<FrP>(w), fe_from<FrP>(EndoK::LAMBDA_M261)), mw);
    uint64_t m[4], kr[4] = { k[0], k[1], k[2], k[3] }, k1[4];
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = (uint64_t)mw[2 * i] | ((uint64_t)mw[2 * i + 1] << 32);
#pragma unroll
    for (int i = 0; i < 5; i++) cond_sub_r(kr); // any 256-bit k: 2^256 < 6 r
    if (!s.neg2) {
        add256(kr, m, k1); // both below r < 2^254
        cond_sub_r(k1);
    } else if (sub256(kr, m, k1)) {
        const uint64_t r[4] = { FrP::P64[0], FrP::P64[1], FrP::P64[2], FrP::P64[3] }, v[4] = { k1[0], k1[1], k1[2], k1[3] };
        add256(v, r, k1);
    }
    s.neg1 = (k1[2] | k1[3]) != 0; // |k1| < 2^128 << r / 2: a residue with high limbs is r - |k1|
    if (s.neg1) {
        const uint64_t r[4] = { FrP::P64[0], FrP::P64[1], FrP::P64[2], FrP::P64[3] }, v[4] = { k1[0], k1[1], k1[2], k1[3] };
        (void)sub256(r, v, k1);
    }
    s.k1[0] = k1[0];
    s.k1[1] = k1[1];
    s.k2[0] = t[0];
    s.k2[1] = t[1];
    s.fits = (k1[2] | k1[3] | t[2] | t[3]) == 0;
}

// ---- the group law on points whose bounds say what the formulas deliver ------------------------------------------------------------------------------------
// Xyzz of g1.hpp types every coordinate as < 12 p; negating such a y would leave the bound the type can carry.  The coordinates the formulas return are
// tighter (X3 a difference below 9 p, the rest fresh products), and with them the operand of an addition may carry a negated y.
struct Pt {
    Fe<Fq, 1, 9> x;
    Fe<Fq, 1, 2> y, zz, zzz;
};
struct Operand {
    Fe<Fq, 1, 9> x;
    Fe<Fq, 1, 3> y;
    Fe<Fq, 1, 2> zz, zzz;
};
// 2 p  [dbl-2008-s-1]; p finite (y != 0 on this curve)
BB_HD void dbl_pt(Pt& p)
{
    auto U = weak(dbl(p.y));
    auto Vv = sqr(U);
    auto W = mul(U, Vv);
    auto S = mul(p.x, Vv);
    auto XX = sqr(p.x);
    auto M = weak(add(dbl(XX), XX));
    auto X3 = weak(sub(sqr(M), dbl(S)));
    auto Y3 = mul_sub(M, sub(S, X3), W, p.y);
    p.zz = mul(Vv, p.zz);
    p.zzz = mul(W, p.zzz);
    p.x = X3;
    p.y = Y3;
}
// acc += q  [add-2008-s], q finite.  The accumulator's infinity is a flag, as in madd_ip: set at the start and by q = -acc, cleared by the first addition.
// acc == q doubles.  All three cases occur: small k, k = lambda +- 1 and k = r - 1 reach them (tests/srs_update_cases.py).
BB_HD void add_pt(Pt& acc, bool& inf, const Operand& q)
{
    if (inf) {
        acc.x = q.x;
        acc.y = mul(q.y, fe_one<Fq>()); // the accumulator's y is typed < 2 p: one product by one brings a negated operand back under it (once per ladder)
        acc.zz = q.zz;
        acc.zzz = q.zzz;
        inf = false;
        return;
    }
    auto U1 = mul(acc.x, q.zz);
    auto U2 = mul(q.x, acc.zz);
    auto S1 = mul(acc.y, q.zzz);
    auto S2 = mul(q.y, acc.zzz);
    auto P = weak(sub(U2, U1));
    auto R = weak(sub(S2, S1));
    auto PP = sqr(P);
    if (is_zero_mulout(PP)) { // same x: rare
        if (is_zero_slow(R)) dbl_pt(acc);
        else inf = true;
        return;
    }
    auto PPP = mul(P, PP);
    auto Q = mul(U1, PP);
    auto X3 = weak(sub(sqr(R), add(PPP, dbl(Q))));
    auto Y3 = mul_sub(R, sub(Q, X3), S1, PPP);
    acc.zz = mul(mul(acc.zz, q.zz), PP);
    acc.zzz = mul(mul(acc.zzz, q.zzz), PPP);
    acc.x = X3;
    acc.y = Y3;
}

// ---- the ladder ---------------------------------------------------------------------------------------------------------------------------------------------
// Fixed windows of WB bits with ODD signed digits (the recoding of groups/wnaf.hpp:15-55 computed from the bits, no digit array): a magnitude is made odd
// by adding one (the skew: that point is subtracted again at the end), then digit j = (u_j | 1) - (u_{j+1} even ? 2^WB : 0) for the windows u_j of the odd
// value, the top one without the borrow.  sum_j d_j 2^(WB j) telescopes back to the value.  Digits are never zero, so every lane of a wave adds in every
// window and the table holds the 2^(WB-1) odd multiples only.  D windows cover 129 bits: a magnitude below 2^128 plus its skew.
template <int WB> struct Ladder {
    static constexpr int NT = 1 << (WB - 1);       // table entries: P, 3 P, ... (2^WB - 1) P
    static constexpr int D = (129 + WB - 1) / WB; // windows
};
BB_HD uint32_t bits_at(uint64_t m0, uint64_t m1, uint64_t m2, int pos) // bits [pos, pos + 32) of a 192-bit value, pos < 192 and wave-uniform
{
    const int l = pos >> 6, sh = pos & 63;
    const uint64_t lo = l == 0 ? m0 : l == 1 ? m1 : m2, hi = l == 0 ? m1 : l == 1 ? m2 : 0;
    uint64_t v = lo >> sh;
    if (sh) v |= hi << (64 - sh);
    return (uint32_t)v;
}
// 1 / a = a^(p - 2); the exponent is read from constants by wave-uniform selects (an indexed local array would live in scratch)
BB_HD Fe<Fq, 1, 2> fq_inverse_fermat(const Fe<Fq, 1, 2>& a)
{
    Fe<Fq, 1, 2> acc = fe_one<Fq>();
#pragma unroll 1
    for (int l = 3; l >= 0; --l) {
        const uint64_t e = l == 3 ? Fq::P64[3] : l == 2 ? Fq::P64[2] : l == 1 ? Fq::P64[1] : Fq::P64[0] - 2;
#pragma unroll 1
        for (int b = 63; b >= 0; --b) {
            acc = sqr(acc);
            if ((e >> b) & 1) acc = mul(acc, a);
        }
    }
    return acc;
}

BB_HD void load_pt(Pt& p, bool& inf, const uint32_t (&w)[32]);
// The base of a ladder is handed in as words and formed inside it, after the split: formed before, it is live across the split and k_srs_update leaves
// its 250 VGPRs (256 + 4 AGPRs, one wave per SIMD).
BB_HD void ladder_base(Pt& t0, const uint32_t (&w)[32]) // a finite scratch point
{
    bool never;
    load_pt(t0, never, w);
}
BB_HD void ladder_base(Pt& t0, const uint32_t (&w)[16]) // a resident row: affine, Montgomery-261, canonical
{
    AffineV<1> p;
    load_affine_m261(p, w);
    t0.x = p.x;
    t0.y = p.y;
    t0.zz = fe_one<Fq>();
    t0.zzz = fe_one<Fq>();
}
// acc = k * base, XYZZ out, no inversion; k a plain integer, any 256-bit value.  base: the 16 words of a resident row or the 32 words of a FINITE scratch
// point, whose own ZZ, ZZZ need not be one (dbl_pt and add_pt carry the denominators); of the group's order, as every point of this curve is (the cofactor
// is one).  inf: the result is infinity (k == 0 mod r), acc then holds nothing.
template <int WB, class Base> BB_HD void ladder_pt(const Base& base, const uint64_t (&k)[4], Pt& acc, bool& inf)
{
    constexpr int NT = Ladder<WB>::NT, D = Ladder<WB>::D;
    // Over an affine base T[0] has ZZ = ZZZ = 1, constants that take no register.  Over a projective one the table would hold 2 NT more field elements than
    // the 250 VGPRs of k_srs_update leave room for (270 registers, one wave per SIMD): there the entries are brought to COMMON denominators, kept in T[0].
    constexpr bool COMMON = std::is_same<Base, uint32_t[32]>::value;
    EndoSplit sp;
    endo_split(k, sp);
    // the two magnitudes made odd: 129 bits each
    const bool skew1 = (sp.k1[0] & 1) == 0, skew2 = (sp.k2[0] & 1) == 0;
    const uint64_t a0 = sp.k1[0] + (skew1 ? 1 : 0), a1 = sp.k1[1] + (uint64_t)(a0 < sp.k1[0]), a2 = (uint64_t)(a1 < sp.k1[1]);
    const uint64_t b0 = sp.k2[0] + (skew2 ? 1 : 0), b1 = sp.k2[1] + (uint64_t)(b0 < sp.k2[0]), b2 = (uint64_t)(b1 < sp.k2[1]);

    // the odd multiples of the row, XYZZ, in registers
    Pt T[NT];
    {
        ladder_base(T[0], base);
        Pt two = T[0];
        dbl_pt(two);
        Operand o2;
        o2.x = two.x;
        o2.y = two.y;
        o2.zz = two.zz;
        o2.zzz = two.zzz;
#pragma unroll
        for (int t = 1; t < NT; t++) {
            T[t] = T[t - 1];
            bool never = false;
            add_pt(T[t], never, o2); // (2 t - 1) P + 2 P: no exceptional case below the group order
        }
    }
    if constexpr (COMMON) {
        // entry t: (X f_t, Y g_t, ZZ f_t, ZZZ g_t) with f_t, g_t the products of the OTHER entries' ZZ and ZZZ -- the same point, f_t^3 = g_t^2 as the
        // formulas need, and every entry now over prod ZZ, prod ZZZ.  Prefix products up, suffix products down: 6 NT - 10 products for the factors, 2 NT to apply.
        Fe<Fq, 1, 2> fz[NT], fw[NT], run_z = T[0].zz, run_w = T[0].zzz;
#pragma unroll
        for (int t = 1; t < NT; t++) {
            fz[t] = run_z;
            fw[t] = run_w;
            run_z = mul(run_z, T[t].zz);
            run_w = mul(run_w, T[t].zzz);
        }
        Fe<Fq, 1, 2> suf_z = T[NT - 1].zz, suf_w = T[NT - 1].zzz;
#pragma unroll
        for (int t = NT - 2; t >= 0; --t) {
            if (t == 0) {
                fz[0] = suf_z;
                fw[0] = suf_w;
            } else {
                fz[t] = mul(fz[t], suf_z);
                fw[t] = mul(fw[t], suf_w);
                suf_z = mul(suf_z, T[t].zz);
                suf_w = mul(suf_w, T[t].zzz);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
            T[t].x = mul(T[t].x, fz[t]);
            T[t].y = mul(T[t].y, fw[t]);
        }
        T[0].zz = run_z;
        T[0].zzz = run_w;
    }
    const FeT<Fq> beta = fe_from<Fq>(Fq::BETA);

    acc = T[0];
    inf = true;
#pragma unroll 1
    for (int j = D - 1; j >= -1; --j) { // j = -1: the two skews
        if (j >= 0 && j != D - 1 && !inf) {
#pragma unroll 1
            for (int t = 0; t < WB; t++) dbl_pt(acc);
        }
#pragma unroll 1
        for (int h = 0; h < 2; h++) { // h = 0: k1 on P; h = 1: k2 on (beta x, -y)
            const uint64_t m0 = h ? b0 : a0, m1 = h ? b1 : a1, m2 = h ? b2 : a2;
            const bool kneg = h ? sp.neg2 : sp.neg1;
            uint32_t idx = 0;
            bool dneg = true, active = h ? skew2 : skew1; // the skew: take the point away once
            if (j >= 0) {
                const uint32_t v = bits_at(m0, m1, m2, j * WB);
                const uint32_t u = (v & ((1u << WB) - 1u)) | 1u;
                dneg = j != D - 1 && ((v >> WB) & 1u) == 0; // the window above is even: it lends 2^WB
                idx = (dneg ? (1u << WB) - u : u) >> 1;
                active = true;
            }
            Operand q;
            q.x = T[0].x;
            Fe<Fq, 1, 2> y = T[0].y;
            q.zz = T[0].zz;
            q.zzz = T[0].zzz;
#pragma unroll
            for (int t = 1; t < NT; t++) {
                const bool take = idx == (uint32_t)t;
#pragma unroll
                for (int l = 0; l < NL; l++) {
                    q.x.d[l] = take ? T[t].x.d[l] : q.x.d[l];
                    y.d[l] = take ? T[t].y.d[l] : y.d[l];
                    if constexpr (!COMMON) {
                        q.zz.d[l] = take ? T[t].zz.d[l] : q.zz.d[l];
                        q.zzz.d[l] = take ? T[t].zzz.d[l] : q.zzz.d[l];
                    }
                }
            }
            if (h) q.x = mul(q.x, beta); // the endomorphism image of a table entry: one product, when it is used
            // the multiple is negative iff kneg != dneg; the image carries -y, so there the positive multiple is the one that negates
            const bool negy = (kneg != dneg) != (h != 0);
            const Fe<Fq, 1, 3> ny = weak(neg(y));
#pragma unroll
            for (int l = 0; l < NL; l++) q.y.d[l] = negy ? ny.d[l] : y.d[l];
            if (active) add_pt(acc, inf, q);
        }
    }
}

// o = k * (the row w), both in the resident form (Montgomery-261, canonical, 16 words); k a plain integer, any 256-bit value, not 0 mod r.
template <int WB> BB_HD void ladder_row(const uint32_t (&w)[16], const uint64_t (&k)[4], uint32_t (&o)[16])
{
    Pt acc;
    bool inf;
    ladder_pt<WB>(w, k, acc, inf);
    // affine: x = X / ZZ, y = Y / ZZZ.  The result is finite: r is prime and k != 0 (mod r), so k P != infinity.  (A lane that ends at infinity all the same --
    // an input row outside the group, which the caller's curve test excludes -- stores a zero row.)
    if (inf) {
#pragma unroll
        for (int t = 0; t < 16; t++) o[t] = 0;
        return;
    }
    const auto inv = fq_inverse_fermat(mul(acc.zz, acc.zzz));
    const auto izz = mul(inv, acc.zzz), izzz = mul(inv, acc.zz);
    store_affine_m261(o, mul(acc.x, izz), mul(acc.y, izzz));
}

// ---- the radix-2 butterfly on points (srs_lagrange.hip) ---------------------------------------------------------------------------------------------------
// A scratch point is 32 words: X, Y, ZZ, ZZZ, Montgomery-261, canonical.  Its infinity flag is ZZ == 0 (all eight words; no finite point has it), and in
// registers a bool beside the Pt, as the ladder's accumulator carries it.
BB_HD void load_pt(Pt& p, bool& inf, const uint32_t (&w)[32])
{
    uint32_t c[8], any = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) any |= w[16 + i];
    inf = any == 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int i = 0; i < 8; i++) c[i] = w[8 * q + i];
        const Fe<Fq, 1, 6> u = unpack<Fq>(c); // stored canonical: the value is below p
#pragma unroll
        for (int l = 0; l < NL; l++) {
            if (q == 0) p.x.d[l] = u.d[l];
            if (q == 1) p.y.d[l] = u.d[l];
            if (q == 2) p.zz.d[l] = u.d[l];
            if (q == 3) p.zzz.d[l] = u.d[l];
        }
    }
}
BB_HD void store_pt(uint32_t (&w)[32], const Pt& p, bool inf)
{
    if (inf) {
#pragma unroll
        for (int i = 0; i < 32; i++) w[i] = 0;
        return;
    }
    uint32_t c[8];
    to_canonical(p.x, c);
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = c[i];
    to_canonical(p.y, c);
#pragma unroll
    for (int i = 0; i < 8; i++) w[8 + i] = c[i];
    to_canonical(p.zz, c);
#pragma unroll
    for (int i = 0; i < 8; i++) w[16 + i] = c[i];
    to_canonical(p.zzz, c);
#pragma unroll
    for (int i = 0; i < 8; i++) w[24 + i] = c[i];
}
// (a, t) -> (a + t, a - t), complete: either may be infinity, t == a doubles the sum and empties the difference, t == -a the other way round
BB_HD void butterfly_pt(Pt& a, bool& ainf, Pt& t, bool& tinf)
{
    if (tinf) { // a + inf = a - inf = a
        t = a;
        tinf = ainf;
        return;
    }
    Operand q;
    q.x = t.x;
    q.zz = t.zz;
    q.zzz = t.zzz;
    const Fe<Fq, 1, 3> ny = weak(neg(t.y));
#pragma unroll
    for (int l = 0; l < NL; l++) q.y.d[l] = ny.d[l];
    Pt d = a;
    bool dinf = ainf;
    add_pt(d, dinf, q);
#pragma unroll
    for (int l = 0; l < NL; l++) q.y.d[l] = t.y.d[l];
    add_pt(a, ainf, q);
    t = d;
    tinf = dinf;
}

// 32 words of a scratch point by four-word vector accesses (16-byte aligned)
BB_HD void load_words32(const uint32_t* p, uint32_t (&w)[32])
{
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint4 v = q[t];
        w[4 * t] = v.x; w[4 * t + 1] = v.y; w[4 * t + 2] = v.z; w[4 * t + 3] = v.w;
    }
}
BB_HD void store_words32(uint32_t* p, const uint32_t (&w)[32])
{
    uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int t = 0; t < 8; t++) q[t] = make_uint4(w[4 * t], w[4 * t + 1], w[4 * t + 2], w[4 * t + 3]);
}
// o <- the affine form of the scratch point w in the reference's format (x, y: Montgomery-256, canonical; infinity: bit 63 of y[3], the rest zero), by one
// Fermat inversion.  The finish kernels of kzg_open_cosets.hip and g1_recover.hip, each with its own indexing, are this.
BB_HD void affine_from_scratch(const uint32_t (&w)[32], uint32_t (&o)[16])
{
    Pt p;
    bool inf;
    load_pt(p, inf, w);
    if (inf) {
#pragma unroll
        for (int t = 0; t < 16; t++) o[t] = 0;
        o[15] = 0x80000000u;
    } else {
        const auto inv = fq_inverse_fermat(mul(p.zz, p.zzz));
        const auto izz = mul(inv, p.zzz), izzz = mul(inv, p.zz);
        uint32_t c[8];
        to_canonical(m261_to_m256<Fq>(mul(p.x, izz)), c);
#pragma unroll
        for (int t = 0; t < 8; t++) o[t] = c[t];
        to_canonical(m261_to_m256<Fq>(mul(p.y, izzz)), c);
#pragma unroll
        for (int t = 0; t < 8; t++) o[8 + t] = c[t];
    }
}
// the butterfly of one lane on its two scratch slots: (a, b) -> (a + k b, a - k b).  unit: k == 1, no ladder (k is not read then).  b is read first and a only
// after the ladder, whose table fills the register file.
template <int WB> BB_HD void butterfly_slots(uint32_t* pa, uint32_t* pb, const uint64_t (&k)[4], bool unit)
{
    uint32_t w[32];
    Pt t, a;
    bool tinf, ainf;
    load_words32(pb, w);
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) any |= w[16 + i];
    if (unit || any == 0) load_pt(t, tinf, w); // a ladder over an infinite base is infinity
    else ladder_pt<WB>(w, k, t, tinf);
    load_words32(pa, w);
    load_pt(a, ainf, w);
    butterfly_pt(a, ainf, t, tinf);
    store_pt(w, a, ainf);
    store_words32(pa, w);
    store_pt(w, t, tinf);
    store_words32(pb, w);
}

} // namespace bbgpu
