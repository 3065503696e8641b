// csrc/host_lagrange_open.hpp (host PRODUCT code: the host twins of bbgpu_fr_evaluate_lagrange_device / bbgpu_kate_opening_lagrange_device) compiled with
// -fsanitize=address,undefined: n = 2 and 64, z off the domain, zero, and on it (first, middle, last element, and a representative lifted by r), batch 1
// and 3, with padding between the polynomials and in place.  Expected values come from the definition without any shortcut: the coefficients by a plain
// O(n^2) inverse transform, Horner evaluation and synthetic division (host_fallback.hpp), and a plain O(n^2) forward transform of the quotient.
// A stand-alone program with its own main; built and run by tests/test_lagrange_open_host.py::test_host_twins_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_fallback.hpp"
#include "../../barretenberg_amd/csrc/host_lagrange_open.hpp"

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

// out_k = scale * sum_i in_i base^(i k)
static std::vector<Fr> dft(const std::vector<Fr>& in, const Fr& base, const Fr& scale)
{
    const size_t n = in.size();
    std::vector<Fr> out(n);
    Fr bk = fr_one();
    for (size_t k = 0; k < n; k++) {
        Fr acc = fr_zero(), p = fr_one();
        for (size_t i = 0; i < n; i++) {
            acc = fr_add(acc, fr_mul(in[i], p));
            p = fr_mul(p, bk);
        }
        out[k] = fr_mul(acc, scale);
        bk = fr_mul(bk, base);
    }
    return out;
}

static void run(size_t n, int batch, size_t stride, const Fr& z, const char* name)
{
    const int lg = lagrange_open_log2(n);
    const Fr w = fr_root_of_unity(lg), pad = fr_from_u64(0x5A5A);
    std::vector<Fr> v((size_t)batch * stride, pad);
    for (int b = 0; b < batch; b++)
        for (size_t i = 0; i < n; i++) v[b * stride + i] = random_fr();
    std::vector<Fr> want_q = v, want_f(batch);
    for (int b = 0; b < batch; b++) {
        const std::vector<Fr> vb(v.begin() + b * stride, v.begin() + b * stride + n);
        std::vector<Fr> c = dft(vb, fr_inv(w), fr_inv(fr_from_u64(n))), q(n);
        want_f[b] = poly_evaluate(c[0].d, n, z);
        const Fr f2 = kate_opening(c[0].d, q[0].d, n, z);
        CHECK(fr_eq(f2, want_f[b]), "%s n=%zu: the two definitions of f(z) differ", name, n);
        const std::vector<Fr> qv = dft(q, w, fr_one());
        for (size_t i = 0; i < n; i++) want_q[b * stride + i] = qv[i];
    }
    std::vector<Fr> f(batch), f2(batch), q = v;
    for (auto& e : q) e = pad; // a destination of its own: only the polynomials' elements may change
    lagrange_open_host(v[0].d, nullptr, n, stride, batch, z, f[0].d);
    for (int b = 0; b < batch; b++) CHECK(fr_eq(f[b], want_f[b]), "%s n=%zu batch %d: evaluation", name, n, b);
    lagrange_open_host(v[0].d, q[0].d, n, stride, batch, z, f2[0].d);
    for (int b = 0; b < batch; b++) CHECK(fr_eq(f2[b], want_f[b]), "%s n=%zu batch %d: f(z) of the opening", name, n, b);
    for (size_t i = 0; i < q.size(); i++) CHECK(fr_eq(q[i], (i % stride) < n ? want_q[i] : pad), "%s n=%zu element %zu: quotient", name, n, i);
    std::vector<Fr> inplace = v;
    lagrange_open_host(inplace[0].d, inplace[0].d, n, stride, batch, z, nullptr); // in place, no f(z) wanted
    for (size_t i = 0; i < q.size(); i++) CHECK(fr_eq(inplace[i], want_q[i]), "%s n=%zu element %zu: quotient in place", name, n, i);
}

int main()
{
    for (size_t n : { (size_t)2, (size_t)64 }) {
        const Fr w = fr_root_of_unity(lagrange_open_log2(n));
        std::vector<std::pair<const char*, Fr>> zs = { { "random", random_fr() }, { "zero", fr_zero() }, { "one", fr_one() }, { "last", fr_pow(w, n - 1) },
                                                       { "middle", fr_pow(w, n / 2) } };
        Fr lifted = fr_pow(w, n / 2 + 1 < n ? n / 2 + 1 : 1); // + r: r < 2^254, so the sum fits
        uint64_t carry = 0;
        for (int i = 0; i < 4; i++) {
            const unsigned __int128 t = (unsigned __int128)lifted.d[i] + bbgpu::FrHostP::P[i] + carry;
            lifted.d[i] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        zs.push_back({ "lifted", lifted });
        for (auto& [name, z] : zs) {
            size_t m = 0;
            const bool on = lagrange_open_on_domain(fr_mul(z, fr_one()), lagrange_open_log2(n), &m);
            CHECK(on == (strcmp(name, "random") && strcmp(name, "zero")), "%s n=%zu: on-domain verdict", name, n);
            if (on) CHECK(fr_eq(fr_pow(w, m), fr_mul(z, fr_one())), "%s n=%zu: m = %zu", name, n, m);
            run(n, 1, n, z, name);
            run(n, 3, n, z, name);
            run(n, 3, n + 5, z, name);
        }
    }
    CHECK(!lagrange_open_sizes_ok(1, 1, 1) && !lagrange_open_sizes_ok(3, 3, 1) && !lagrange_open_sizes_ok((size_t)1 << 25, (size_t)1 << 25, 1), "sizes");
    CHECK(!lagrange_open_sizes_ok(8, 7, 1) && !lagrange_open_sizes_ok(8, 8, 0) && !lagrange_open_sizes_ok(8, 8, 65) && lagrange_open_sizes_ok(8, 8, 64), "sizes");
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
