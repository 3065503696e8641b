// Host twins of the fold and of a folded opening (csrc/host_lagrange_open.hpp: fold_host, lagrange_open_folded_host) under AddressSanitizer and
// UndefinedBehaviorSanitizer.  The expected values come from linearity: the quotient of F = sum_b gamma_b f_b is sum_b gamma_b q_b and F(z) is
// sum_b gamma_b f_b(z), with q_b and f_b(z) from the unfolded twin (itself held to the coefficient form by tests/cpp/test_lagrange_open_host.cpp) --
// at z on the domain too, where element m of the quotient is defined through a sum over the others.
// A stand-alone program with its own main; built and run by tests/test_opening_session_host.py::test_host_twins_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_lagrange_open.hpp"

using namespace bbgpu::host;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("MISMATCH %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); fails++; } } while (0)

static uint64_t rng_state = 0xD1B54A32D192ED03ULL;
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

static void run(size_t n, int batch, size_t stride, const Fr& z, const char* name)
{
    const Fr pad = fr_from_u64(0x5A5A);
    std::vector<Fr> v((size_t)batch * stride, pad), gamma(batch);
    for (int b = 0; b < batch; b++) {
        gamma[b] = b == 1 ? fr_zero() : random_fr();
        for (size_t i = 0; i < n; i++) v[b * stride + i] = random_fr();
    }
    const std::vector<Fr> kept = v;
    // by linearity, from the unfolded twin
    std::vector<Fr> q = v, f(batch), want_q(n, fr_zero()), want_fold(n, fr_zero());
    Fr want_f = fr_zero();
    lagrange_open_host(v[0].d, q[0].d, n, stride, batch, z, f[0].d);
    for (int b = 0; b < batch; b++) {
        want_f = fr_add(want_f, fr_mul(gamma[b], f[b]));
        for (size_t i = 0; i < n; i++) {
            want_q[i] = fr_add(want_q[i], fr_mul(gamma[b], q[b * stride + i]));
            want_fold[i] = fr_add(want_fold[i], fr_mul(v[b * stride + i], fr_mul(gamma[b], fr_one()))); // (one operand of fr_mul must be below r)
        }
    }
    std::vector<Fr> got(n + 1, pad), got_q(n + 1, pad); // one element of guard behind each
    Fr got_f;
    fold_host(got[0].d, v[0].d, n, stride, batch, gamma[0].d, false);
    for (size_t i = 0; i < n; i++) CHECK(fr_eq(got[i], want_fold[i]), "%s n=%zu element %zu: fold", name, n, i);
    lagrange_open_folded_host(v[0].d, n, stride, batch, gamma[0].d, z, got_q[0].d, false, got_f.d);
    CHECK(fr_eq(got_f, want_f), "%s n=%zu: F(z)", name, n);
    for (size_t i = 0; i < n; i++) CHECK(fr_eq(got_q[i], want_q[i]), "%s n=%zu element %zu: folded quotient", name, n, i);
    // accumulate: a second call doubles both; F(z) stays that of the call alone; no f wanted
    fold_host(got[0].d, v[0].d, n, stride, batch, gamma[0].d, true);
    lagrange_open_folded_host(v[0].d, n, stride, batch, gamma[0].d, z, got_q[0].d, true, nullptr);
    for (size_t i = 0; i < n; i++) {
        CHECK(fr_eq(got[i], fr_add(want_fold[i], want_fold[i])), "%s n=%zu element %zu: fold, accumulated", name, n, i);
        CHECK(fr_eq(got_q[i], fr_add(want_q[i], want_q[i])), "%s n=%zu element %zu: folded quotient, accumulated", name, n, i);
    }
    CHECK(fr_eq(got[n], pad) && fr_eq(got_q[n], pad), "%s n=%zu: written past n", name, n);
    for (size_t i = 0; i < v.size(); i++) CHECK(fr_eq(v[i], kept[i]), "%s n=%zu: the values were written", name, n);
}

int main()
{
    for (size_t n : { (size_t)2, (size_t)64 }) {
        const Fr w = fr_root_of_unity(lagrange_open_log2(n));
        const std::vector<std::pair<const char*, Fr>> zs = { { "random", random_fr() }, { "zero", fr_zero() }, { "one", fr_one() }, { "last", fr_pow(w, n - 1) },
                                                             { "middle", fr_pow(w, n / 2) } };
        for (auto& [name, z] : zs) {
            run(n, 1, n, z, name);
            run(n, 3, n, z, name);
            run(n, 3, n + 5, z, name);
        }
    }
    { // the fold alone takes any length
        std::vector<Fr> v(2 * 7), g = { random_fr(), random_fr() }, out(5);
        for (auto& e : v) e = random_fr();
        fold_host(out[0].d, v[0].d, 5, 7, 2, g[0].d, false);
        for (size_t i = 0; i < 5; i++) CHECK(fr_eq(out[i], fr_add(fr_mul(v[i], fr_mul(g[0], fr_one())), fr_mul(v[7 + i], fr_mul(g[1], fr_one())))), "fold of 5 elements, element %zu", i);
    }
    CHECK(fold_sizes_ok(1, 1, 1) && fold_sizes_ok(1000, 1000, 64) && !fold_sizes_ok(0, 0, 1) && !fold_sizes_ok(((size_t)1 << 24) + 1, (size_t)1 << 25, 1), "sizes");
    CHECK(!fold_sizes_ok(8, 7, 1) && !fold_sizes_ok(8, 8, 0) && !fold_sizes_ok(8, 8, 65), "sizes");
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
