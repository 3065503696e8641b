// The host twin of bbgpu_kzg_open_cosets_device (csrc/host_kzg_open_cosets.hpp: kzg_open_cosets_setup_host, kzg_open_cosets_proofs_host) under
// AddressSanitizer and UndefinedBehaviorSanitizer, at (n, l) = (8, 2), (16, 4) and (128, 64).  The expected proofs come from the quotient definition, coset
// by coset: q_k with f = q_k (X^l - psi^k) + r_k by synthetic division, committed by the bucket method over the same rows.  Batch 1 and 3, with padding
// between the polynomials; a polynomial of degree below l (every proof at infinity) and one whose residues 0 and 1 give the same point at every frequency.
// A stand-alone program with its own main; built and run by tests/test_kzg_open_cosets_host.py::test_host_twin_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_kzg_open_cosets.hpp"

using namespace bbgpu::host;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("MISMATCH %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); fails++; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static Fr random_fr()
{
    Fr a;
    for (int i = 0; i < 4; i++) a.d[i] = rng();
    return a; // any representative below 2^256
}

// the endo table of x^j G, j < n: only the even entries are read
static std::vector<uint64_t> make_table(size_t n, const Fr& x)
{
    std::vector<uint64_t> table(16 * n, 0);
    const Xyzz g = { FQ_ONE, fq_dbl(FQ_ONE), FQ_ONE, FQ_ONE };
    Fr k = fr_one();
    for (size_t j = 0; j < n; j++) {
        uint64_t o[12];
        g1_to_normalised(g1_times_plain(g, fr_from_mont(k)), o);
        memcpy(&table[16 * j], o, 64);
        k = fr_mul(k, x);
    }
    return table;
}

static void run(const std::vector<uint64_t>& table, const Fr& x, size_t n, size_t l, int batch, size_t stride, int kind, const char* name)
{
    int log2n, log2l;
    CHECK(kzg_open_cosets_log2(n, l, &log2n, &log2l), "%s (%zu, %zu): sizes", name, n, l);
    const size_t m = n / l;
    const Fr pad = fr_from_u64(0x5A5A), xinv = fr_inv(x);
    std::vector<Fr> c((size_t)batch * stride, pad);
    for (int b = 0; b < batch; b++)
        for (size_t j = 0; j < n; j++) {
            Fr v = random_fr();
            if (kind == 1) v = j < l ? v : fr_zero();                              // degree < l
            if (kind == 2 && j % l == 1) v = fr_mul(c[b * stride + j - 1], xinv); // c^(1) = x^-1 c^(0): residues 0 and 1 give equal points
            c[b * stride + j] = v;
        }
    const std::vector<Fr> kept = c;
    std::vector<Xyzz> S;
    uint64_t bad = ~0ull;
    CHECK(kzg_open_cosets_setup_host(table.data(), log2n, log2l, S, &bad) == BBGPU_OK, "%s (%zu, %zu): setup", name, n, l);
    std::vector<uint64_t> got((size_t)batch * m * 8 + 8, 0xA5A5A5A5A5A5A5A5ULL); // one point of guard behind
    kzg_open_cosets_proofs_host(S, log2n, log2l, c[0].d, stride, batch, got.data());
    const Fr psi = fr_root_of_unity(log2n - log2l);
    std::vector<Fr> q(n);
    for (int b = 0; b < batch; b++) {
        Fr z = fr_one();
        for (size_t k = 0; k < m; k++) {
            for (size_t d = n; d-- > 0;) // q_d = c_(d+l) + z q_(d+l), zero from n - l on
                q[d] = d + l < n ? fr_add(fr_mul(c[b * stride + d + l], fr_one()), fr_mul(z, q[d + l])) : fr_zero();
            uint64_t want[12];
            g1_to_normalised(msm_pippenger(q[0].d, table.data(), n, 16), want);
            CHECK(!memcmp(&got[((size_t)b * m + k) * 8], want, 64), "%s (%zu, %zu) polynomial %d coset %zu", name, n, l, b, k);
            if (kind == 1) CHECK(got[((size_t)b * m + k) * 8 + 7] == 1ULL << 63, "%s (%zu, %zu): degree below l opens to infinity", name, n, l);
            z = fr_mul(z, psi);
        }
    }
    for (size_t k = 0; k < 8; k++) CHECK(got[(size_t)batch * m * 8 + k] == 0xA5A5A5A5A5A5A5A5ULL, "%s (%zu, %zu): written past the proofs", name, n, l);
    for (size_t i = 0; i < c.size(); i++) CHECK(fr_eq(c[i], kept[i]), "%s (%zu, %zu): the coefficients were written", name, n, l);
}

int main()
{
    const Fr x = fr_mul(random_fr(), fr_one());
    const size_t sizes[3][2] = { { 8, 2 }, { 16, 4 }, { 128, 64 } };
    const std::vector<uint64_t> table = make_table(128, x);
    for (const auto& s : sizes) {
        run(table, x, s[0], s[1], 1, s[0], 0, "random");
        run(table, x, s[0], s[1], 3, s[0] + 5, 0, "random, padded");
        run(table, x, s[0], s[1], 1, s[0], 1, "degree < l");
        run(table, x, s[0], s[1], 1, s[0], 2, "equal residues");
    }
    { // the first row off the curve is named; rows from n - l on are not read
        std::vector<uint64_t> bad_table(table.begin(), table.begin() + 16 * 16);
        bad_table[16 * 13 + 4] ^= 1;
        std::vector<Xyzz> S;
        uint64_t bad = ~0ull;
        CHECK(kzg_open_cosets_setup_host(bad_table.data(), 4, 2, S, &bad) == BBGPU_OK, "row 13 of (16, 4) is not read");
        bad_table[16 * 11 + 4] ^= 1;
        bad_table[16 * 3 + 4] ^= 1;
        CHECK(kzg_open_cosets_setup_host(bad_table.data(), 4, 2, S, &bad) == BBGPU_ERR_ARG && bad == 3, "bad row %llu", (unsigned long long)bad);
    }
    int a, b;
    CHECK(kzg_open_cosets_log2(2, 1, &a, &b) && a == 1 && b == 0 && kzg_open_cosets_log2((size_t)1 << 21, 64, &a, &b) && a == 21 && b == 6 &&
              !kzg_open_cosets_log2(2, 2, &a, &b) && !kzg_open_cosets_log2(256, 128, &a, &b) && !kzg_open_cosets_log2(16, 0, &a, &b) &&
              !kzg_open_cosets_log2(16, 3, &a, &b) && !kzg_open_cosets_log2(12, 4, &a, &b) && !kzg_open_cosets_log2((size_t)1 << 22, 64, &a, &b),
          "sizes");
    CHECK(kzg_open_cosets_t_source(0, 4, 4, 1) == 13 && kzg_open_cosets_t_source(5, 4, 4, 1) == -1 && kzg_open_cosets_t_source(6, 4, 4, 1) == 5 &&
              kzg_open_cosets_t_source(7, 4, 4, 3) == 11,
          "t source");
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
