// csrc/host_pairing.hpp and csrc/host_srs_check.hpp (host PRODUCT code: the BN254 pairing and the host side of the SRS check) compiled with
// -fsanitize=address,undefined and driven against the reference's known answer (tests/golden/pairing_kats.json, a data fixture; its path is argv[1]) and the
// oracle's G1 arithmetic (oracle/bn254_oracle.c; test infrastructure).  Built and run by tests/test_pairing_host.py::test_pairing_code_under_sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_pairing.hpp"
#include "../../barretenberg_amd/csrc/host_srs_check.hpp"
#include "../../oracle/bn254_oracle.h"

using namespace bbgpu::host;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); fails++; } } while (0)

// every "0x..." token of the fixture in file order: per known answer 8 limbs of p, 16 of q, 48 of e
static std::vector<uint64_t> read_hex_words(const char* path)
{
    std::vector<uint64_t> out;
    FILE* f = fopen(path, "rb");
    if (!f) return out;
    std::vector<char> text;
    char buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + k);
    fclose(f);
    text.push_back(0);
    for (const char* c = text.data(); (c = strstr(c, "\"0x")) != nullptr; c += 3) out.push_back(strtoull(c + 1, nullptr, 16));
    return out;
}

static void to_mont(const uint64_t* plain, size_t count, uint64_t* out)
{
    for (size_t i = 0; i < count; i++) orc_to_mont(ORC_FQ, plain + 4 * i, out + 4 * i);
}
static Fq12 pair(const uint64_t p[8], const G2Affine& q)
{
    uint64_t qw[16];
    memcpy(qw, &q, 128);
    return pairing_product(p, qw, 1);
}

int main(int argc, char** argv)
{
    // ---- the reference's constant, byte for byte
    const std::vector<uint64_t> kat = read_hex_words(argc > 1 ? argv[1] : "tests/golden/pairing_kats.json");
    CHECK(kat.size() >= 72 && kat.size() % 72 == 0, "fixture: %zu words", kat.size());
    for (size_t k = 0; k + 72 <= kat.size(); k += 72) {
        uint64_t p[8], q[16], want[48];
        to_mont(&kat[k], 2, p);
        to_mont(&kat[k + 8], 4, q);
        to_mont(&kat[k + 24], 12, want);
        const Fq12 got = pairing_product(p, q, 1);
        CHECK(!memcmp(&got, want, 384), "pairing differs from the reference's constant");
        CHECK(g2_on_curve(g2_from_words(q)) && g2_has_order_r(g2_from_words(q)), "the constant's Q is not in G2");
    }
    // ---- bilinearity: e(aP, bQ) == e(abP, Q) == e(P, abQ), non-degeneracy, infinity, the product form
    uint64_t g[8];
    orc_g1_one_affine(g);
    for (int t = 0; t < 3; t++) {
        uint64_t ab[8], prod[4], aP[12], abP[12];
        orc_random_scalars(900 + t, 2, ab);
        orc_mul(ORC_FR, ab, ab + 4, prod);
        orc_g1_scalar_mul(g, ab, aP);
        orc_g1_scalar_mul(g, prod, abP);
        Fr b, abf;
        memcpy(b.d, ab + 4, 32);
        memcpy(abf.d, prod, 32);
        G2Affine bQ, abQ;
        CHECK(g2_scalar_mul_affine(G2_ONE, b, &bQ) && g2_scalar_mul_affine(G2_ONE, abf, &abQ), "G2 multiple");
        const Fq12 e1 = pair(aP, bQ), e2 = pair(abP, G2_ONE), e3 = pair(g, abQ);
        CHECK(fq12_eq(e1, e2) && fq12_eq(e1, e3), "bilinearity case %d", t);
        CHECK(!fq12_eq(e1, fq12_one()), "degenerate pairing case %d", t);
        uint64_t two[16], qq[32];
        memcpy(two, aP, 64);
        orc_g1_neg_affine(aP, two + 8);
        memcpy(qq, &bQ, 128);
        memcpy(qq + 16, &bQ, 128);
        CHECK(fq12_eq(pairing_product(two, qq, 2), fq12_one()), "e(P, Q) e(-P, Q) != 1 case %d", t);
        uint64_t inf[8] = { 0, 0, 0, 0, 0, 0, 0, 1ULL << 63 };
        CHECK(fq12_eq(pair(inf, bQ), fq12_one()), "e(infinity, Q) != 1");
    }
    // ---- the SRS check on the host at n = 64: honest, a negated row located, a wrong x G2, a row off the curve
    {
        const size_t N = 64;
        std::vector<uint64_t> srs(8 * N), table(16 * N);
        uint64_t x[4], x1[4];
        orc_random_scalars(4242, 1, x);
        orc_add(ORC_FR, x, orc_const(ORC_FR, "one"), x1);
        orc_make_srs(x, N, srs.data());
        orc_generate_point_table(srs.data(), table.data(), N);
        Fr xf, x1f;
        memcpy(xf.d, x, 32);
        memcpy(x1f.d, x1, 32);
        G2Affine xg2, x1g2;
        CHECK(g2_scalar_mul_affine(G2_ONE, xf, &xg2) && g2_scalar_mul_affine(G2_ONE, x1f, &x1g2), "x G2");
        uint64_t g2x[16], g2x1[16];
        memcpy(g2x, &xg2, 128);
        memcpy(g2x1, &x1g2, 128);
        const uint64_t seed[4] = { 1, 2, 3, 4 };
        bbgpu_srs_report R, R2;
        CHECK(srs_check_host(table.data(), N, g2x, seed, BBGPU_SRS_CHECK_LOCATE, &R) == 0, "rc");
        CHECK(R.n == N && R.bad_points == 0 && R.first_bad_point == UINT64_MAX && R.first_is_generator == 1 && R.g2_ok == 1 && R.powers_checked == 1 &&
                  R.powers_ok == 1 && R.first_bad_power == UINT64_MAX, "honest table: bad %llu g2 %u checked %u ok %u", (unsigned long long)R.bad_points, R.g2_ok,
              R.powers_checked, R.powers_ok);
        CHECK(srs_check_host(table.data(), N, g2x, seed, 0, &R2) == 0 && !memcmp(&R, &R2, sizeof R), "two runs with one seed differ");
        CHECK(srs_check_host(table.data(), N, g2x1, seed, BBGPU_SRS_CHECK_LOCATE, &R) == 0 && R.g2_ok == 1 && R.powers_checked == 1 && R.powers_ok == 0 &&
                  R.first_bad_power == 0, "x + 1: ok %u first %llu", R.powers_ok, (unsigned long long)R.first_bad_power);
        std::vector<uint64_t> bad = table;
        orc_neg(ORC_FQ, &table[16 * 37 + 4], &bad[16 * 37 + 4]);
        CHECK(srs_check_host(bad.data(), N, g2x, seed, BBGPU_SRS_CHECK_LOCATE, &R) == 0 && R.bad_points == 0 && R.powers_ok == 0 && R.first_bad_power == 36,
              "negated row 37: bad %llu ok %u first %llu", (unsigned long long)R.bad_points, R.powers_ok, (unsigned long long)R.first_bad_power);
        bad = table;
        bad[16 * 5 + 4] += 1;
        CHECK(srs_check_host(bad.data(), N, g2x, seed, 0, &R) == 0 && R.bad_points == 1 && R.first_bad_point == 5 && R.powers_checked == 0, "row 5 off the curve");
        g2x[8] += 1;
        CHECK(srs_check_host(table.data(), N, g2x, seed, 0, &R) == 0 && R.g2_ok == 0 && R.powers_checked == 0, "x G2 off the twist");
        uint64_t s1[4], s2[4];
        CHECK(srs_check_seed(nullptr, s1) && srs_check_seed(nullptr, s2) && memcmp(s1, s2, 32), "two drawn seeds are equal");
    }
    if (fails) {
        printf("%d FAILURES\n", fails);
        return 1;
    }
    printf("ALL OK\n");
    return 0;
}
