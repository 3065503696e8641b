// The butterfly of csrc/srs_lagrange.hip's stage kernel (csrc/g1_ladder.hpp butterfly_slots: the ladder over a PROJECTIVE base with its table brought to
// common denominators, no inversion, then the complete (a + t, a - t)) run on the CPU as a stand-alone program (own main; tests/test_srs_lagrange_host.py
// builds it with the host sanitizers) and compared, after normalisation, with a plain double-and-add and the complete additions of host_g1.hpp.
// Bases: projective (ZZ != 1) and infinite; a: projective, infinite, equal to t (the sum doubles, the difference is infinity), equal to -t (the other way
// round); twiddles: 1 (with and without the ladder), r - 1, lambda +- 1, lambda, r - lambda, 2^128, a scalar whose split has a negative half, 1000 random.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include "../../barretenberg_amd/csrc/g1_ladder.hpp"
#include "../../barretenberg_amd/csrc/host_g1.hpp"
using namespace bbgpu;
static uint64_t rng = 88172645463325252ULL;
static uint64_t next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

struct alignas(16) Slot {
    uint32_t w[32];
};
// host coordinate (Montgomery 2^256, canonical) <-> eight words of a scratch point (Montgomery 2^261, canonical)
static void to_words(const host::Fq& v, uint32_t* w8)
{
    uint32_t in[8], out[8];
    memcpy(in, v.d, 32);
    to_canonical(m256_to_m261<Fq>(unpack<Fq>(in)), out);
    memcpy(w8, out, 32);
}
static host::Fq from_words(const uint32_t* w8)
{
    uint32_t in[8], out[8];
    memcpy(in, w8, 32);
    to_canonical(m261_to_m256<Fq>(unpack<Fq>(in)), out);
    host::Fq v;
    memcpy(v.d, out, 32);
    return v;
}
static Slot to_slot(const host::Xyzz& p)
{
    Slot s;
    memset(&s, 0, sizeof s);
    if (host::g1_is_inf(p)) return s;
    to_words(p.x, s.w);
    to_words(p.y, s.w + 8);
    to_words(p.zz, s.w + 16);
    to_words(p.zzz, s.w + 24);
    return s;
}
static host::Xyzz from_slot(const Slot& s)
{
    host::Xyzz p = { from_words(s.w), from_words(s.w + 8), from_words(s.w + 16), from_words(s.w + 24) };
    return p;
}
static host::Xyzz times(const host::Xyzz& p, const uint64_t k[4])
{
    host::Xyzz acc = host::g1_infinity();
    for (int i = 255; i >= 0; --i) {
        acc = host::g1_dbl(acc);
        if ((k[i >> 6] >> (i & 63)) & 1) acc = host::g1_add(acc, p);
    }
    return acc;
}
static host::Xyzz negated(const host::Xyzz& p)
{
    host::Xyzz r = p;
    const host::Fq zero = { { 0, 0, 0, 0 } };
    if (!host::g1_is_inf(p)) r.y = host::fq_sub(zero, p.y);
    return r;
}
// the same point over another denominator: (X z^2, Y z^3, ZZ z^2, ZZZ z^3)
static host::Xyzz rescaled(const host::Xyzz& p, const host::Fq& z)
{
    const host::Fq z2 = host::fq_sqr(z), z3 = host::fq_mul(z2, z);
    host::Xyzz r = { host::fq_mul(p.x, z2), host::fq_mul(p.y, z3), host::fq_mul(p.zz, z2), host::fq_mul(p.zzz, z3) };
    return r;
}
static bool same_point(const host::Xyzz& a, const host::Xyzz& b)
{
    uint64_t x[12], y[12];
    host::g1_to_normalised(a, x);
    host::g1_to_normalised(b, y);
    return !memcmp(x, y, 96);
}

int main()
{
    const uint64_t R[4] = { FrP::P64[0], FrP::P64[1], FrP::P64[2], FrP::P64[3] };
    const uint64_t LAM[4] = { 0x8b17ea66b99c90ddULL, 0x5bfc41088d8daaa7ULL, 0xb3c4d79d41a91758ULL, 0 };
    auto addk = [&](const uint64_t a[4], int64_t d, uint64_t out[4]) { // a + d, small d
        unsigned __int128 c = 0;
        const uint64_t hi = d < 0 ? ~0ULL : 0, dd[4] = { (uint64_t)d, hi, hi, hi };
        for (int i = 0; i < 4; i++) { c += (unsigned __int128)a[i] + dd[i]; out[i] = (uint64_t)c; c >>= 64; }
    };
    host::Xyzz G;
    G.x = host::FQ_ONE; G.y = host::fq_dbl(host::FQ_ONE); G.zz = host::FQ_ONE; G.zzz = host::FQ_ONE;
    const uint64_t seven[4] = { 7, 0, 0, 0 }, eleven[4] = { 11, 0, 0, 0 };
    host::Fq z1 = { { next(), next(), next(), next() >> 4 } }, z2 = { { next(), next(), next(), next() >> 4 } };
    const host::Xyzz B = rescaled(times(G, seven), z1), A = rescaled(times(G, eleven), z2); // projective, ZZ != 1

    int bad = 0, cases = 0, doubled = 0, emptied = 0, negative_half = 0;
    // one butterfly: slots (a, b), twiddle k; unit: the kernel's skip of the ladder
    auto check = [&](const host::Xyzz& a, const host::Xyzz& b, const uint64_t k[4], bool unit, const char* what) {
        Slot sa = to_slot(a), sb = to_slot(b);
        const uint64_t kk[4] = { k[0], k[1], k[2], k[3] };
        butterfly_slots<3>(sa.w, sb.w, kk, unit);
        const host::Xyzz t = times(b, k), sum = host::g1_add(a, t), dif = host::g1_add(a, negated(t));
        const host::Xyzz gs = from_slot(sa), gd = from_slot(sb);
        cases++;
        if (!same_point(gs, sum) || !same_point(gd, dif)) {
            bad++;
            if (bad < 10) printf("MISMATCH %s k=%016lx%016lx%016lx%016lx\n", what, k[3], k[2], k[1], k[0]);
        }
        // an infinite result is stored as the flag alone
        for (const Slot* s : { &sa, &sb }) {
            uint32_t zz = 0, any = 0;
            for (int i = 0; i < 8; i++) zz |= s->w[16 + i];
            for (int i = 0; i < 32; i++) any |= s->w[i];
            if (zz == 0 && any != 0) { bad++; printf("infinity with data %s\n", what); }
        }
    };
    auto all_pairs = [&](const uint64_t k[4], bool unit) {
        const host::Xyzz inf = host::g1_infinity(), t = times(B, k);
        check(A, B, k, unit, "proj/proj");
        check(inf, B, k, unit, "inf/proj");
        check(A, inf, k, unit, "proj/inf");
        check(inf, inf, k, unit, "inf/inf");
        check(rescaled(t, z2), B, k, unit, "a = t");  // the sum doubles, the difference is infinity
        check(rescaled(negated(t), z2), B, k, unit, "a = -t");
        doubled += 2;
        emptied += 2;
    };
    uint64_t k[4] = { 1, 0, 0, 0 };
    all_pairs(k, true);  // twiddle 1, the ladder skipped
    all_pairs(k, false); // twiddle 1 through the ladder
    addk(R, -1, k); all_pairs(k, false);
    addk(R, -2, k); all_pairs(k, false);
    for (int d = -1; d <= 1; d++) { addk(LAM, d, k); all_pairs(k, false); }
    { uint64_t rl[4]; uint64_t borrow = 0;
      for (int i = 0; i < 4; i++) { unsigned __int128 t = (unsigned __int128)R[i] - LAM[i] - borrow; rl[i] = (uint64_t)t; borrow = (t >> 64) ? 1 : 0; }
      all_pairs(rl, false); }
    k[0] = 0; k[1] = 0; k[2] = 1; k[3] = 0; all_pairs(k, false); // 2^128
    k[0] = 2; k[1] = k[2] = k[3] = 0; all_pairs(k, false);
    // scalars whose split has a negative half: k = ceil(j 2^256 / g2), as tests/cpp/test_srs_update_ladder.hip finds them
    for (int i = 0; i < 64 && negative_half < 4; i++) {
        const unsigned __int128 g2 = ((unsigned __int128)2 << 64) | 0xd91d232ec7e0b3d7ULL;
        unsigned __int128 rem = (unsigned __int128)(i + 1);
        uint64_t q[4];
        for (int l = 3; l >= 0; --l) {
            uint64_t ql = 0;
            for (int b = 63; b >= 0; --b) { rem <<= 1; ql <<= 1; if (rem >= g2) { rem -= g2; ql |= 1; } }
            q[l] = ql;
        }
        if (rem) addk(q, 1, q);
        EndoSplit sp; endo_split(q, sp);
        if (sp.neg2) { negative_half++; all_pairs(q, false); }
    }
    if (negative_half == 0) { printf("no scalar with a negative half was tried\n"); bad++; }
    for (int i = 0; i < 1000; i++) {
        k[0] = next(); k[1] = next(); k[2] = next(); k[3] = next() & 0x1fffffffffffffffULL;
        const host::Fq z = { { next(), next(), next(), next() >> 4 } };
        check(rescaled(A, z), rescaled(B, z), k, false, "random");
    }
    printf("%d butterflies (%d with a = +-t, %d scalars with a negative half), %d bad\n", cases, doubled, negative_half, bad);
    if (!bad) printf("ok\n");
    return bad ? 1 : 0;
}
