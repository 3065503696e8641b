// The host twins of bbgpu_g1_ntt and bbgpu_g1_recover (csrc/host_g1_recover.hpp: g1_ntt_verdict, g1_ntt_host, g1_recover_verdict, g1_recover_host) under
// AddressSanitizer and UndefinedBehaviorSanitizer, at (n, d) = (8, 4) and (64, 17), batch 3: columns of multiples of the generator whose scalars are the
// values of polynomials of degree < d (Horner's rule, never a transform), one column with a point at infinity.  The transform there and back returns the
// column; the decoder returns every point from the rows that are listed, top first, with every other row or the first rows missing; one altered point
// shows with redundancy and not without; refused calls write nothing.  A stand-alone program with its own main; built and run by
// tests/test_g1_recover_host.py::test_host_twins_under_sanitizers.
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
static Fr random_fr()
{
    Fr a;
    for (int i = 0; i < 4; i++) a.d[i] = rng();
    return fr_mul(a, fr_one()); // canonical
}
static const uint64_t FILL = 0xA5A5A5A5A5A5A5A5ULL;

static void point_of(const Fr& v, uint64_t out[8])
{
    uint64_t g[8];
    g1_generator_words(g);
    g1_to_words(g1_times_plain(g1_from_words(g), fr_from_mont(v)), out);
}

// all: batch x n x 8 words, column b the values of a polynomial of degree < d times the generator; column 1 has a root at omega^2 (infinity there)
static std::vector<uint64_t> columns(size_t n, size_t d, int batch)
{
    int log2n = 0;
    while (((size_t)1 << log2n) < n) log2n++;
    const Fr w = fr_root_of_unity(log2n);
    std::vector<uint64_t> all((size_t)batch * n * 8);
    for (int b = 0; b < batch; b++) {
        std::vector<Fr> c(d);
        for (Fr& v : c) v = random_fr();
        auto value = [&](size_t i) {
            const Fr x = fr_pow(w, i);
            Fr acc = fr_zero();
            for (size_t k = d; k-- > 0;) acc = fr_add(fr_mul(acc, x), c[k]);
            return acc;
        };
        if (b == 1) c[0] = fr_sub(c[0], value(2));
        for (size_t i = 0; i < n; i++) point_of(value(i), &all[((size_t)b * n + i) * 8]);
    }
    CHECK(g1_words_is_inf(&all[(n + 2) * 8]), "column 1 has no point at infinity");
    return all;
}

static void transforms(size_t n, size_t d)
{
    const int batch = 3;
    const std::vector<uint64_t> all = columns(n, d, batch);
    std::vector<uint64_t> work = all;
    char why[320] = "";
    int log2n = 0;
    int rc = g1_ntt_verdict("test", work.data(), work.data(), n, batch, BBGPU_FFT, &log2n, why, sizeof why);
    CHECK(rc == BBGPU_OK && ((size_t)1 << log2n) == n, "n = %zu: verdict %d %s", n, rc, why);
    if (rc) return;
    g1_ntt_host(work.data(), work.data(), log2n, batch, BBGPU_FFT); // in place
    CHECK(work != all, "n = %zu: the transform changed nothing", n);
    g1_ntt_host(work.data(), work.data(), log2n, batch, BBGPU_IFFT);
    CHECK(work == all, "n = %zu: there and back", n);
    std::vector<uint64_t> coeffs(all.size());
    g1_ntt_host(all.data(), coeffs.data(), log2n, batch, BBGPU_IFFT);
    for (int b = 0; b < batch; b++)
        for (size_t j = d; j < n; j++) CHECK(g1_words_is_inf(&coeffs[((size_t)b * n + j) * 8]), "n = %zu: coefficient %zu of column %d", n, j, b);
}

// mu rows missing: every other row if that gives mu of them, else the first mu; alter: the first listed point of column 1 gets the generator added
static void recover(size_t n, size_t d, size_t mu, bool alter, const char* what)
{
    const int batch = 3;
    const std::vector<uint64_t> all = columns(n, d, batch);
    std::vector<bool> gone(n, false);
    for (size_t i = 0; i < mu; i++) gone[2 * mu <= n ? 2 * i : i] = true;
    std::vector<uint32_t> row;
    for (size_t k = n; k-- > 0;)
        if (!gone[k]) row.push_back((uint32_t)k);
    const size_t count = row.size();
    std::vector<uint64_t> points((size_t)batch * count * 8);
    for (int b = 0; b < batch; b++)
        for (size_t t = 0; t < count; t++) memcpy(&points[((size_t)b * count + t) * 8], &all[((size_t)b * n + row[t]) * 8], 64);
    if (alter) {
        uint64_t g[8];
        g1_generator_words(g);
        g1_to_words(g1_add(g1_from_words(&points[count * 8]), g1_from_words(g)), &points[count * 8]);
    }
    const std::vector<uint64_t> kept = points;
    std::vector<uint64_t> out((size_t)batch * n * 8 + 8, FILL);
    bbgpu_g1_recover_report rep;
    memset(&rep, 0xEE, sizeof rep);
    KzgRecoverShape S;
    char why[320] = "";
    int rc = g1_recover_verdict("test", row.data(), count, points.data(), n, d, batch, out.data(), &rep, &S, why, sizeof why);
    CHECK(rc == BBGPU_OK && S.mu == mu && S.m == n && S.missing.size() == mu, "%s: verdict %d %s", what, rc, why);
    if (rc) return;
    rc = g1_recover_host(S, row.data(), count, points.data(), d, batch, out.data(), &rep, why, sizeof why);
    CHECK(rc == BBGPU_OK, "%s: %d %s", what, rc, why);
    CHECK(points == kept, "%s: the points were written to", what);
    const bool seen = alter && count > d;
    CHECK(rep.missing == mu && rep.consistent == (seen ? 0u : 1u) && rep.first_bad_column == (seen ? 1u : 0u) &&
              (seen ? rep.first_bad_coeff >= d && rep.first_bad_coeff < count : rep.first_bad_coeff == 0),
          "%s: report %u %u %llu %llu", what, rep.consistent, rep.first_bad_column, (unsigned long long)rep.first_bad_coeff, (unsigned long long)rep.missing);
    for (int b = 0; b < batch; b++) {
        if (b != 1 || !alter) CHECK(!memcmp(&out[(size_t)b * n * 8], &all[(size_t)b * n * 8], n * 64), "%s: column %d", what, b);
        else
            for (size_t t = 0; t < count; t++) // the listed points come back as they were given
                CHECK(!memcmp(&out[((size_t)b * n + row[t]) * 8], &points[((size_t)b * count + t) * 8], 64), "%s: point (%d, %zu)", what, b, t);
    }
    for (size_t i = 0; i < 8; i++) CHECK(out[(size_t)batch * n * 8 + i] == FILL, "%s: written past the end", what);
}

static void refused(size_t n, size_t d, const std::vector<uint32_t>& row, int batch, int spoil, int want, const char* text, const char* what)
{
    std::vector<uint64_t> points(((size_t)(batch > 0 ? batch : 1) * row.size() + 1) * 8), out(64, FILL);
    for (size_t i = 0; i * 8 < points.size(); i++) point_of(fr_from_u64(i + 1), &points[i * 8]);
    if (spoil == 1) points[8 * 4] ^= 1;           // off the curve
    if (spoil == 2) points[8 * 4 + 7] |= 1ULL << 63; // the flag of infinity over other words
    bbgpu_g1_recover_report rep;
    KzgRecoverShape S;
    char why[320] = "";
    const int rc = g1_recover_verdict("test", row.data(), row.size(), points.data(), n, d, batch, out.data(), &rep, &S, why, sizeof why);
    CHECK(rc == want && strstr(why, text), "%s: %d, want %d (%s)", what, rc, want, why);
    for (uint64_t v : out) CHECK(v == FILL, "%s: output written", what);
}

int main()
{
    const size_t sizes[2][2] = { { 8, 4 }, { 64, 17 } };
    for (const auto& s : sizes) {
        const size_t n = s[0], d = s[1];
        transforms(n, d);
        recover(n, d, 0, false, "no row missing");
        recover(n, d, 1, false, "one row missing");
        recover(n, d, n - d, false, "as many as d allows");
        recover(n, d, 1, true, "one altered point among redundant rows");
        recover(n, d, n - d, true, "one altered point, no redundancy");
    }
    refused(12, 4, { 0, 1, 2, 3 }, 1, 0, BBGPU_ERR_SIZE, "power of two", "n not a power of two");
    refused(8, 0, { 0, 1, 2, 3 }, 1, 0, BBGPU_ERR_SIZE, "degree bound 0", "degree bound 0");
    refused(8, 9, { 0, 1, 2, 3 }, 1, 0, BBGPU_ERR_SIZE, "degree bound 9", "degree bound above n");
    refused(8, 5, { 0, 1, 2, 3 }, 1, 0, BBGPU_ERR_SIZE, "4 rows", "too few rows");
    refused(8, 4, { 0, 1, 2, 3 }, 0, 0, BBGPU_ERR_SIZE, "batch 0", "batch 0");
    refused(8, 4, { 0, 1, 2, 8 }, 1, 0, BBGPU_ERR_ARG, "row[3] = 8", "a row that does not exist");
    refused(8, 4, { 0, 1, 2, 1 }, 1, 0, BBGPU_ERR_ARG, "row[3] = 1 is listed twice", "a row listed twice");
    refused(8, 4, { 0, 1, 2, 3 }, 2, 1, BBGPU_ERR_ARG, "position 0 of column 1 (row 0)", "a point off the curve");
    refused(8, 4, { 0, 1, 2, 3 }, 2, 2, BBGPU_ERR_ARG, "position 0 of column 1 (row 0)", "a flag of infinity over other words");
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
