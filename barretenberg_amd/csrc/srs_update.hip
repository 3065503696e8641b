// srs_update.hip -- the device part of bbgpu_srs_update (include/bbgpu.h): row i of a resident table becomes y^(first_power + i) * P_i, one lane per row.
// The reference has no such operation (its strings come from a file, io.hpp:159-181); what it has is the pieces: the endomorphism split of a scalar
// (fields/field.hpp:413-485, restated for the host in host_wnaf.hpp) and fixed windows of odd signed digits (groups/wnaf.hpp:15-55).  Here both run per
// lane: k = y^e as a plain integer, k = k1 - lambda k2 with |k1|, |k2| < 2^128, then ONE ladder over both halves -- k P = k1 P + k2 (beta x, -y), since
// (beta x, -y) = -lambda P under Fq::BETA and the lambda of host_wnaf.hpp (checked against the oracle, tests/test_srs_update_host.py) -- so 126 shared
// doublings instead of 254.  The curve test, the G2 half and the registration of the new table are capi.hip's.
#include <hip/hip_runtime.h>

#include "bbgpu_internal.h"
#include "g1.hpp"

namespace bbgpu {

#define HIPCHK(x)                                                                                                      \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) {                                                                                        \
            set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));                                \
            return BBGPU_ERR_HIP;                                                                                      \
        }                                                                                                              \
    } while (0)

namespace {

using Fr = FrP;
constexpr int UT = 64; // threads per workgroup: one wave, as srs_gen_points_kernel (250 VGPRs: two waves per SIMD whatever the workgroup)

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
    const uint64_t r[4] = { Fr::P64[0], Fr::P64[1], Fr::P64[2], Fr::P64[3] };
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
    to_canonical(mul(unpack<Fr>(w), fe_from<Fr>(EndoK::LAMBDA_M261)), mw);
    uint64_t m[4], kr[4] = { k[0], k[1], k[2], k[3] }, k1[4];
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = (uint64_t)mw[2 * i] | ((uint64_t)mw[2 * i + 1] << 32);
#pragma unroll
    for (int i = 0; i < 5; i++) cond_sub_r(kr); // any 256-bit k: 2^256 < 6 r
    if (!s.neg2) {
        add256(kr, m, k1); // both below r < 2^254
        cond_sub_r(k1);
    } else if (sub256(kr, m, k1)) {
        const uint64_t r[4] = { Fr::P64[0], Fr::P64[1], Fr::P64[2], Fr::P64[3] }, v[4] = { k1[0], k1[1], k1[2], k1[3] };
        add256(v, r, k1);
    }
    s.neg1 = (k1[2] | k1[3]) != 0; // |k1| < 2^128 << r / 2: a residue with high limbs is r - |k1|
    if (s.neg1) {
        const uint64_t r[4] = { Fr::P64[0], Fr::P64[1], Fr::P64[2], Fr::P64[3] }, v[4] = { k1[0], k1[1], k1[2], k1[3] };
        (void)sub256(r, v, k1);
    }
    s.k1[0] = k1[0];
    s.k1[1] = k1[1];
    s.k2[0] = t[0];
    s.k2[1] = t[1];
    s.fits = (k1[2] | k1[3] | t[2] | t[3]) == 0;
}
BB_HD void endo_split_words(const uint64_t* k_in, uint64_t* out6)
{
    const uint64_t k[4] = { k_in[0], k_in[1], k_in[2], k_in[3] };
    EndoSplit s;
    endo_split(k, s);
    out6[0] = s.k1[0];
    out6[1] = s.k1[1];
    out6[2] = s.k2[0];
    out6[3] = s.k2[1];
    out6[4] = (s.neg1 ? 1u : 0u) | (s.neg2 ? 2u : 0u) | (s.fits ? 0u : 4u);
    out6[5] = 0;
}
__global__ void __launch_bounds__(UT) k_selftest_endo_split(const uint64_t* __restrict__ k, uint64_t n, uint64_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    endo_split_words(k + 4 * i, out + 6 * i);
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

// o = k * (the row w), both in the resident form (Montgomery-261, canonical, 16 words); k a plain integer, any 256-bit value, not 0 mod r.
// __host__ __device__ like the field code under it, so that the same ladder runs on the CPU against the host group law.
template <int WB> BB_HD void ladder_row(const uint32_t (&w)[16], const uint64_t (&k)[4], uint32_t (&o)[16])
{
    constexpr int NT = Ladder<WB>::NT, D = Ladder<WB>::D;
    EndoSplit sp;
    endo_split(k, sp);
    // the two magnitudes made odd: 129 bits each
    const bool skew1 = (sp.k1[0] & 1) == 0, skew2 = (sp.k2[0] & 1) == 0;
    const uint64_t a0 = sp.k1[0] + (skew1 ? 1 : 0), a1 = sp.k1[1] + (uint64_t)(a0 < sp.k1[0]), a2 = (uint64_t)(a1 < sp.k1[1]);
    const uint64_t b0 = sp.k2[0] + (skew2 ? 1 : 0), b1 = sp.k2[1] + (uint64_t)(b0 < sp.k2[0]), b2 = (uint64_t)(b1 < sp.k2[1]);

    // the odd multiples of the row, XYZZ, in registers
    Pt T[NT];
    {
        AffineV<1> p;
        load_affine_m261(p, w);
        T[0].x = p.x;
        T[0].y = p.y;
        T[0].zz = fe_one<Fq>();
        T[0].zzz = fe_one<Fq>();
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
    const FeT<Fq> beta = fe_from<Fq>(Fq::BETA);

    Pt acc = T[0];
    bool inf = true;
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
                    q.zz.d[l] = take ? T[t].zz.d[l] : q.zz.d[l];
                    q.zzz.d[l] = take ? T[t].zzz.d[l] : q.zzz.d[l];
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

// out[i] = y^(first_power + i) * in[i]; in and out may not overlap
template <int WB>
__global__ void __launch_bounds__(UT) k_srs_update(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n, uint64_t first_power, Limbs9 y261)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // s = y^(first_power + i) in Fr (Montgomery-261), then the plain canonical integer -- as srs_gen_points_kernel
    uint64_t k[4];
    {
        Fe<Fr, 1, 2> s = fe_one<Fr>(), b = fe_from<Fr>(y261.d);
        for (uint64_t e = first_power + i; e; e >>= 1) {
            if (e & 1) s = mul(s, b);
            b = sqr(b);
        }
        FeT<Fr> one_raw = fe_zero<Fr>();
        one_raw.d[0] = 1;
        uint32_t kw[8];
        to_canonical(mul(s, one_raw), kw);
#pragma unroll
        for (int t = 0; t < 4; t++) k[t] = (uint64_t)kw[2 * t] | ((uint64_t)kw[2 * t + 1] << 32);
    }
    uint32_t w[16], o[16];
    const uint4* src = reinterpret_cast<const uint4*>(in + i * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint4 v = src[t];
        w[4 * t] = v.x; w[4 * t + 1] = v.y; w[4 * t + 2] = v.z; w[4 * t + 3] = v.w;
    }
    ladder_row<WB>(w, k, o);
    uint4* dst = reinterpret_cast<uint4*>(out + i * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) dst[t] = make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
}

// 3-bit windows: four table entries, 250 VGPRs, no scratch, two waves per SIMD: 16.4 ms per 2^20 rows.  2-bit windows (two entries, 178 VGPRs, still two
// waves) pay 42 more additions per row: 19.9 ms; 4-bit windows (eight entries) need 256 VGPRs and 140 AGPRs of spills and leave one wave per SIMD: 17.7 ms
// (profiles/srs_update.txt).
constexpr int SRS_UPDATE_WB = 3;

} // namespace

// d_in: n resident rows; *d_out_rows: a new allocation of n rows, the caller's on success; host_table_out (may be null): the 2n-entry endo table of the new
// rows, through the export kernel of bbgpu_srs_generate.  y_mont256: Montgomery 2^256, any representative.  first_power + n <= 2^32 (the caller checks).
// kernel_ms (may be null): the device time of k_srs_update alone, from a pair of events around it (bbgpu_set_timing).
int srs_update_rows(const uint32_t* d_in, size_t n, uint64_t first_power, const uint64_t* y_mont256, uint32_t** d_out_rows, uint64_t* host_table_out, hipStream_t st,
                    float* kernel_ms)
{
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events()
        {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } ev;
    if (kernel_ms) {
        HIPCHK(hipEventCreate(&ev.a));
        HIPCHK(hipEventCreate(&ev.b));
    }
    DevBuf rows;
    HIPCHK(dev_malloc(&rows.p, n * 64));
    // y: Montgomery 2^256 -> 2^261, canonical limbs
    uint32_t w[8];
    for (int i = 0; i < 4; i++) { w[2 * i] = (uint32_t)y_mont256[i]; w[2 * i + 1] = (uint32_t)(y_mont256[i] >> 32); }
    Fe<Fr, 1, 2> y261 = m256_to_m261<Fr>(unpack<Fr>(w));
    uint32_t cw[8];
    to_canonical(y261, cw);
    Fe<Fr, 1, 6> yc = unpack<Fr>(cw);
    Limbs9 yl;
    for (int i = 0; i < NL; i++) yl.d[i] = yc.d[i];
    const uint32_t blocks = (uint32_t)((n + UT - 1) / UT); // n <= 2^32: at most 2^26 workgroups
    if (kernel_ms) HIPCHK(hipEventRecord(ev.a, st));
    k_srs_update<SRS_UPDATE_WB><<<blocks, UT, 0, st>>>(d_in, rows.as<uint32_t>(), (uint64_t)n, first_power, yl);
    HIPCHK(launch_check());
    if (kernel_ms) HIPCHK(hipEventRecord(ev.b, st));
    if (host_table_out) {
        DevBuf exp;
        HIPCHK(dev_malloc(&exp.p, n * 128));
        if (int rc = srs_export(rows.as<uint32_t>(), n, exp.as<uint32_t>(), st)) return rc;
        if (int rc = device_to_host_sync(host_table_out, exp.p, n * 128, st)) return rc;
    }
    HIPCHK(hipStreamSynchronize(st));
    if (kernel_ms) HIPCHK(hipEventElapsedTime(kernel_ms, ev.a, ev.b));
    *d_out_rows = rows.release<uint32_t>();
    return BBGPU_OK;
}

} // namespace bbgpu

using namespace bbgpu;

#pragma GCC visibility push(default)
extern "C" {

int bbgpu_selftest_endo_split(int on_device, const uint64_t* k, size_t n, uint64_t* out)
{
    if (!k || !out || n == 0 || n > (1u << 20)) return BBGPU_ERR_ARG;
    if (!on_device) {
        for (size_t i = 0; i < n; i++) endo_split_words(k + 4 * i, out + 6 * i);
        return BBGPU_OK;
    }
    if (bbgpu_device_count() == 0) {
        set_error("no HIP device available: libbbgpu has no CPU fallback");
        return BBGPU_ERR_HIP;
    }
    uint64_t *dk = nullptr, *dout = nullptr;
    int rc = BBGPU_ERR_HIP;
    do {
        if (hipMalloc((void**)&dk, n * 32) != hipSuccess || hipMalloc((void**)&dout, n * 48) != hipSuccess) break;
        if (hipMemcpy(dk, k, n * 32, hipMemcpyHostToDevice) != hipSuccess) break;
        k_selftest_endo_split<<<(uint32_t)((n + UT - 1) / UT), UT>>>(dk, (uint64_t)n, dout);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out, dout, n * 48, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = BBGPU_OK;
    } while (0);
    if (rc) set_error("selftest: HIP failure (%s)", hipGetErrorString(hipGetLastError()));
    if (dk) (void)hipFree(dk);
    if (dout) (void)hipFree(dout);
    return rc;
}

} // extern "C"
#pragma GCC visibility pop
