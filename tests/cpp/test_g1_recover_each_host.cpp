// The host twin of bbgpu_g1_recover_each (csrc/host_g1_recover.hpp: g1_recover_each_verdict, g1_recover_each_host) under AddressSanitizer and
// UndefinedBehaviorSanitizer, at (n, d) = (8, 4) with 0, 1, 2, 3, 4 rows missing and (64, 17) with 0, 1, 30, 47: columns of multiples of the generator whose
// scalars are the values of polynomials of degree < d (Horner's rule, never a transform), every column with its own rows, listed top first.  The decoder
// returns every point of every column; one altered point shows in its column's entry of first_bad where the column has redundancy; refused calls write
// nothing.  A stand-alone program with its own main; built and run by tests/test_g1_recover_each_host.py::test_host_twin_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_g1_recover.hpp"

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
static const uint64_t FILL = 0xA5A5A5A5A5A5A5A5ULL;

// batch x n x 8 words: column b the values of a random polynomial of degree < d times the generator
static std::vector<uint64_t> columns(size_t n, size_t d, int batch)
{
    int log2n = 0;
    while (((size_t)1 << log2n) < n) log2n++;
    const Fr w = fr_root_of_unity(log2n);
    uint64_t g[8];
    g1_generator_words(g);
    std::vector<uint64_t> all((size_t)batch * n * 8);
    for (int b = 0; b < batch; b++) {
        std::vector<Fr> c(d);
        for (Fr& v : c) {
            for (int i = 0; i < 4; i++) v.d[i] = rng();
            v = fr_mul(v, fr_one()); // canonical
        }
        for (size_t i = 0; i < n; i++) {
            const Fr x = fr_pow(w, i);
            Fr acc = fr_zero();
            for (size_t k = d; k-- > 0;) acc = fr_add(fr_mul(acc, x), c[k]);
            g1_to_words(g1_times_plain(g1_from_words(g), fr_from_mont(acc)), &all[((size_t)b * n + i) * 8]);
        }
    }
    return all;
}

static void run(size_t n, size_t d, const std::vector<size_t>& mus)
{
    const int batch = (int)mus.size();
    std::vector<uint64_t> all = columns(n, d, batch);
    std::vector<uint32_t> off(1, 0), row;
    for (int b = 0; b < batch; b++) { // column b misses the mus[b] rows from b on (wrapping), and lists the others top first
        for (size_t k = n; k-- > 0;)
            if ((k + n - (size_t)b) % n >= mus[(size_t)b]) row.push_back((uint32_t)k);
        off.push_back((uint32_t)row.size());
    }
    auto gather = [&](std::vector<uint64_t>& pts) {
        pts.resize(row.size() * 8);
        for (int b = 0; b < batch; b++)
            for (uint32_t t = off[(size_t)b]; t < off[(size_t)b + 1]; t++) memcpy(&pts[(size_t)t * 8], &all[((size_t)b * n + row[t]) * 8], 64);
    };
    std::vector<uint64_t> pts, out((size_t)batch * n * 8, FILL), first_bad((size_t)batch, FILL);
    gather(pts);
    KzgRecoverEachShape S;
    bbgpu_g1_recover_each_report rep;
    char why[320];
    int rc = g1_recover_each_verdict("test", off.data(), row.data(), pts.data(), n, d, batch, out.data(), &rep, &S, why, sizeof why);
    CHECK(rc == BBGPU_OK, "n %zu: the verdict refuses a good call: %s", n, why);
    rc = g1_recover_each_host(S, off.data(), row.data(), pts.data(), d, batch, out.data(), first_bad.data(), &rep, why, sizeof why);
    CHECK(rc == BBGPU_OK && rep.consistent == 1 && out == all, "n %zu: the columns are not recovered", n);
    for (int b = 0; b < batch; b++) CHECK(first_bad[(size_t)b] == ~0ull, "n %zu column %d: a finding in an honest column", n, b);
    // P + G at the first listed point of column 1 (one row missing: redundancy) and of the last column (count == d: none)
    for (int b : { 1, batch - 1 }) {
        std::vector<uint64_t> bad = pts;
        uint64_t g[8];
        g1_generator_words(g);
        uint64_t* p = &bad[(size_t)off[(size_t)b] * 8];
        g1_to_words(g1_add(g1_from_words(p), g1_from_words(g)), p);
        rc = g1_recover_each_verdict("test", off.data(), row.data(), bad.data(), n, d, batch, out.data(), &rep, &S, why, sizeof why);
        if (rc == BBGPU_OK) rc = g1_recover_each_host(S, off.data(), row.data(), bad.data(), d, batch, out.data(), nullptr, &rep, why, sizeof why);
        const bool seen = n - mus[(size_t)b] > d;
        CHECK(rc == BBGPU_OK && rep.consistent == (seen ? 0u : 1u) && (!seen || rep.first_bad_column == (uint32_t)b), "n %zu column %d: altered point, consistent %u",
              n, b, rep.consistent);
    }
    // refused calls write nothing
    std::vector<uint64_t> kept(out.size(), FILL);
    out = kept;
    bbgpu_g1_recover_each_report untouched;
    memset(&untouched, 0x5A, sizeof untouched);
    rep = untouched;
    std::vector<uint32_t> twice = row;
    twice[off[1]] = twice[off[1] + 1];
    CHECK(g1_recover_each_verdict("test", off.data(), twice.data(), pts.data(), n, d, batch, out.data(), &rep, &S, why, sizeof why) == BBGPU_ERR_ARG, "a row listed twice");
    CHECK(g1_recover_each_verdict("test", off.data(), row.data(), pts.data(), n, n + 1, batch, out.data(), &rep, &S, why, sizeof why) == BBGPU_ERR_SIZE, "degree bound");
    CHECK(g1_recover_each_verdict("test", off.data(), row.data(), pts.data(), n, d + 1, batch, out.data(), &rep, &S, why, sizeof why) == BBGPU_ERR_SIZE, "too few rows");
    CHECK(out == kept && memcmp(&rep, &untouched, sizeof rep) == 0, "n %zu: a refused call wrote something", n);
}

int main()
{
    run(8, 4, { 0, 1, 2, 3, 4 });
    run(64, 17, { 0, 1, 30, 47 });
    printf(fails ? "FAILED %d\n" : "ok\n", fails);
    return fails != 0;
}
