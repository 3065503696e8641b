// The row ladder of csrc/srs_update.hip (k_srs_update's body: endomorphism split, odd signed windows over both halves, complete additions, the Fermat
// inversion) run on the CPU as a stand-alone program (own main; tests/test_srs_update_host.py builds it with the host sanitizers) and compared, row for
// row, with a plain double-and-add on host_g1.hpp: small k, r - k, lambda +- d, r - lambda +- d, every 2^b and 2^b +- 1, 3000 random scalars and the
// scalars just above multiples of 2^256 / g2 whose split has a negative half -- at the kernel's 3-bit windows.
// The translation unit is included whole: the ladder lives in its anonymous namespace.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "../../barretenberg_amd/csrc/srs_update.hip"
#include "../../barretenberg_amd/csrc/host_g1.hpp"
#include "../../barretenberg_amd/csrc/host_fr.hpp"
namespace bbgpu {
void set_error(const char*, ...) {}
hipError_t dev_malloc(void**, size_t) { return hipErrorUnknown; }
hipError_t dev_free(void*) { return hipSuccess; }
hipError_t launch_check() { return hipSuccess; }
int device_to_host_sync(void*, const void*, size_t, hipStream_t, bool*) { return -1; }
int srs_export(const uint32_t*, size_t, uint32_t*, hipStream_t) { return -1; }
}
extern "C" int bbgpu_device_count(void) { return 0; }
using namespace bbgpu;
static uint64_t rng = 88172645463325252ULL;
static uint64_t next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }
template <int WB> static int run()
{
    const uint64_t R[4] = { FrP::P64[0], FrP::P64[1], FrP::P64[2], FrP::P64[3] };
    const uint64_t LAM[4] = { 0x8b17ea66b99c90ddULL, 0x5bfc41088d8daaa7ULL, 0xb3c4d79d41a91758ULL, 0 };
    // a base point: 7 G by the host law
    host::Xyzz G;
    G.x = host::FQ_ONE; G.y = host::fq_dbl(host::FQ_ONE); G.zz = host::FQ_ONE; G.zzz = host::FQ_ONE;
    host::Xyzz B = host::g1_infinity();
    for (int i = 0; i < 7; i++) B = host::g1_add(B, G);
    uint64_t bn[12];
    host::g1_to_normalised(B, bn);
    memcpy(B.x.d, bn, 32); memcpy(B.y.d, bn + 4, 32); B.zz = host::FQ_ONE; B.zzz = host::FQ_ONE;
    // resident form of the base
    uint32_t w16[16], wr[16];
    memcpy(w16, bn, 64);
    AffineV<2> a; load_affine_m256(a, w16); store_affine_m261(wr, a.x, a.y);
    int bad = 0, cases = 0;
    auto check = [&](const uint64_t k[4]) {
        uint64_t kk[4] = { k[0], k[1], k[2], k[3] };
        uint32_t o[16];
        ladder_row<WB>(wr, kk, o);
        host::Xyzz acc = host::g1_infinity();
        for (int i = 255; i >= 0; --i) { acc = host::g1_dbl(acc); if ((k[i >> 6] >> (i & 63)) & 1) acc = host::g1_add(acc, B); }
        uint64_t want[12]; host::g1_to_normalised(acc, want);
        AffineV<1> r; load_affine_m261(r, o);
        uint32_t gx[8], gy[8];
        to_canonical(m261_to_m256<Fq>(r.x), gx); to_canonical(m261_to_m256<Fq>(r.y), gy);
        cases++;
        if (memcmp(gx, want, 32) || memcmp(gy, want + 4, 32)) { bad++; if (bad < 10) printf("WB=%d MISMATCH k=%016lx%016lx%016lx%016lx\n", WB, k[3], k[2], k[1], k[0]); }
    };
    auto addk = [&](const uint64_t a[4], int64_t d, uint64_t out[4]) { // a + d, small d
        unsigned __int128 c = 0; uint64_t dd[4] = { (uint64_t)d, d < 0 ? ~0ULL : 0, d < 0 ? ~0ULL : 0, d < 0 ? ~0ULL : 0 };
        for (int i = 0; i < 4; i++) { c += (unsigned __int128)a[i] + dd[i]; out[i] = (uint64_t)c; c >>= 64; }
    };
    uint64_t k[4];
    for (uint64_t s = 1; s <= 40; s++) { k[0] = s; k[1] = k[2] = k[3] = 0; check(k); }
    for (int d = -40; d <= -1; d++) { addk(R, d, k); check(k); }
    for (int d = -20; d <= 20; d++) { addk(LAM, d, k); check(k); }
    { uint64_t rl[4]; uint64_t borrow = 0; for (int i = 0; i < 4; i++) { unsigned __int128 t = (unsigned __int128)R[i] - LAM[i] - borrow; rl[i] = (uint64_t)t; borrow = (t >> 64) ? 1 : 0; }
      for (int d = -20; d <= 20; d++) { addk(rl, d, k); check(k); } }
    for (int b = 1; b < 254; b++) { memset(k, 0, 32); k[b >> 6] = 1ULL << (b & 63); check(k); uint64_t k2[4]; addk(k, -1, k2); check(k2); addk(k, 1, k2); check(k2); }
    for (int i = 0; i < 3000; i++) { k[0] = next(); k[1] = next(); k[2] = next(); k[3] = next() & 0x1fffffffffffffffULL; check(k); }
    // scalars with negative t: search near multiples of 2^256 / g2 by probing the split itself
    int negs = 0;
    for (int i = 0; i < 64; i++) {
        // k = ceil(j 2^256 / g2) for j = i + 1 computed by long division in 128-bit pieces
        const unsigned __int128 g2 = ((unsigned __int128)2 << 64) | 0xd91d232ec7e0b3d7ULL;
        unsigned __int128 rem = (unsigned __int128)(i + 1);
        uint64_t q[4];
        for (int l = 3; l >= 0; --l) { // divide (rem << 64) by g2, 64 bits at a time, bitwise
            uint64_t ql = 0;
            for (int b = 63; b >= 0; --b) { rem <<= 1; ql <<= 1; if (rem >= g2) { rem -= g2; ql |= 1; } }
            q[l] = ql;
        }
        if (rem) addk(q, 1, q);
        EndoSplit sp; endo_split(q, sp);
        if (sp.neg1 || sp.neg2) { negs++; check(q); }
        if (!sp.fits) { printf("does not fit\n"); bad++; }
    }
    if (negs == 0) { printf("no scalar with a negative half was tried\n"); bad++; }
    printf("WB=%d: %d cases (%d with a negative half), %d bad\n", WB, cases, negs, bad);
    return bad;
}
int main()
{
    int b = run<3>();
    if (!b) printf("ok\n");
    return b ? 1 : 0;
}
