// The host twin of bbgpu_kzg_open_all_device -- the twin of the coset entries at coset size 1 without a bound (csrc/host_kzg_open_cosets.hpp:
// kzg_open_cosets_setup_bounded_host, kzg_open_cosets_proofs_bounded_host at log2l = 0, log2d = log2n) -- under AddressSanitizer and
// UndefinedBehaviorSanitizer, at n = 8 and n = 64.  The expected proofs come from the quotient definition, point by point: the coefficients of
// (f(X) - f(w^i)) / (X - w^i) by kate_opening (host_fallback.hpp), committed by the bucket method over the same rows.  Batch 1 and 3, with padding between
// the polynomials; a constant polynomial (every proof at infinity), f = X (every proof the generator) and a polynomial with a zero among t^.
// A stand-alone program with its own main; built and run by tests/test_kzg_open_all_host.py::test_host_twin_under_sanitizers.
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

static void run(const std::vector<uint64_t>& table, size_t n, int batch, size_t stride, int kind, const char* name)
{
    const int log2n = kzg_open_all_log2(n);
    const Fr pad = fr_from_u64(0x5A5A);
    std::vector<Fr> c((size_t)batch * stride, pad);
    for (int b = 0; b < batch; b++)
        for (size_t j = 0; j < n; j++) {
            Fr v = random_fr();
            if (kind == 1) v = j == 0 ? v : fr_zero();                        // constant
            if (kind == 2) v = j == 1 ? fr_one() : fr_zero();                 // X
            if (kind == 3) v = (j == 1 || j == n - 1) ? fr_one() : fr_zero(); // X + X^(n-1): t^_k = 0 at k = n/2 and 3n/2
            c[b * stride + j] = v;
        }
    const std::vector<Fr> kept = c;
    std::vector<Xyzz> S;
    uint64_t bad = ~0ull;
    CHECK(kzg_open_cosets_setup_bounded_host(table.data(), log2n, 0, S, &bad) == BBGPU_OK, "%s n=%zu: setup", name, n);
    std::vector<uint64_t> got((size_t)batch * n * 8 + 8, 0xA5A5A5A5A5A5A5A5ULL); // one point of guard behind
    kzg_open_cosets_proofs_bounded_host(S, log2n, 0, log2n, c[0].d, stride, batch, got.data());
    const Fr w = fr_root_of_unity(log2n);
    std::vector<Fr> q(n);
    for (int b = 0; b < batch; b++) {
        Fr z = fr_one();
        for (size_t i = 0; i < n; i++) {
            (void)kate_opening(c[b * stride].d, q[0].d, n, z);
            uint64_t want[12];
            g1_to_normalised(msm_pippenger(q[0].d, table.data(), n, 16), want);
            CHECK(!memcmp(&got[((size_t)b * n + i) * 8], want, 64), "%s n=%zu polynomial %d point %zu", name, n, b, i);
            if (kind == 1) CHECK(got[((size_t)b * n + i) * 8 + 7] == 1ULL << 63, "%s n=%zu: a constant opens to infinity", name, n);
            if (kind == 2) CHECK(!memcmp(&got[((size_t)b * n + i) * 8], table.data(), 64), "%s n=%zu: X opens to the generator", name, n);
            z = fr_mul(z, w);
        }
    }
    for (size_t k = 0; k < 8; k++) CHECK(got[(size_t)batch * n * 8 + k] == 0xA5A5A5A5A5A5A5A5ULL, "%s n=%zu: written past the proofs", name, n);
    for (size_t i = 0; i < c.size(); i++) CHECK(fr_eq(c[i], kept[i]), "%s n=%zu: the coefficients were written", name, n);
}

int main()
{
    const Fr x = fr_mul(random_fr(), fr_one());
    for (size_t n : { (size_t)8, (size_t)64 }) {
        const std::vector<uint64_t> table = make_table(n, x);
        run(table, n, 1, n, 0, "random");
        run(table, n, 3, n + 5, 0, "random, padded");
        run(table, n, 1, n, 1, "constant");
        run(table, n, 1, n, 2, "X");
        run(table, n, 1, n, 3, "X + X^(n-1)");
    }
    { // a row off the curve is named
        std::vector<uint64_t> table = make_table(8, x);
        table[16 * 3 + 4] ^= 1;
        std::vector<Xyzz> S;
        uint64_t bad = ~0ull;
        CHECK(kzg_open_cosets_setup_bounded_host(table.data(), 3, 0, S, &bad) == BBGPU_ERR_ARG && bad == 3, "bad row %llu", (unsigned long long)bad);
    }
    CHECK(kzg_open_all_log2(2) == 1 && kzg_open_all_log2((size_t)1 << 21) == 21 && kzg_open_all_log2((size_t)1 << 22) < 0 && kzg_open_all_log2(1) < 0 &&
              kzg_open_all_log2(0) < 0 && kzg_open_all_log2(6) < 0, "log2");
    CHECK(kzg_open_all_sizes_ok(8, 8, 1) && kzg_open_all_sizes_ok(8, 9, 64) && !kzg_open_all_sizes_ok(8, 7, 1) && !kzg_open_all_sizes_ok(8, 8, 0) &&
              !kzg_open_all_sizes_ok(8, 8, 65) && kzg_open_all_sizes_ok((size_t)1 << 21, (size_t)1 << 21, 1) &&
              !kzg_open_all_sizes_ok((size_t)1 << 21, (size_t)1 << 21, 2) && kzg_open_all_sizes_ok((size_t)1 << 15, (size_t)1 << 15, 64),
          "sizes");
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
