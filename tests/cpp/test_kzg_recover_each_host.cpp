// The host twin of bbgpu_kzg_recover_cells_each (csrc/host_kzg_recover_each.hpp: kzg_recover_each_verdict, kzg_recover_cells_each_host) under
// AddressSanitizer and UndefinedBehaviorSanitizer, at (n, l) = (16, 4) and (64, 1): batch 3, every polynomial with a set of its own -- no cell missing, one
// missing, as many as the degree bound allows -- listed from the top, with padding between the polynomials that must stay as it was.  The expected
// coefficients are those of the polynomials the cells were made from (values by Horner's rule, never a transform); then one altered value in polynomial
// 1, and refused calls, which write nothing.  A stand-alone program with its own main; built and run by
// tests/test_kzg_recover_each_host.py::test_host_twin_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_kzg_recover_each.hpp"

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

// polynomial b misses mu[b] cells: every other cell from b while that gives mu[b] of them, else the first mu[b]; alter: polynomial 1's first value gets one added
static void run(size_t n, size_t l, size_t d, const std::vector<size_t>& mu, size_t stride, bool alter, const char* what)
{
    const size_t m = n / l;
    const int batch = (int)mu.size();
    int log2n = 0;
    while (((size_t)1 << log2n) < n) log2n++;
    const Fr w = fr_root_of_unity(log2n);
    std::vector<uint32_t> off(1, 0), cell;
    for (int b = 0; b < batch; b++) {
        std::vector<bool> gone(m, false);
        for (size_t i = 0; i < mu[b]; i++) gone[2 * mu[b] + b <= m ? 2 * i + b : i] = true;
        for (size_t k = m; k-- > 0;)
            if (!gone[k]) cell.push_back((uint32_t)k);
        off.push_back((uint32_t)cell.size());
        CHECK(off[b + 1] - off[b] == m - mu[b], "%s: cell list %d", what, b);
    }
    std::vector<Fr> coeffs((size_t)batch * n, fr_zero());
    std::vector<uint64_t> values(cell.size() * l * 4);
    for (int b = 0; b < batch; b++) {
        Fr* c = &coeffs[(size_t)b * n];
        for (size_t i = 0; i < d; i++) c[i] = random_fr();
        for (size_t t = off[b]; t < off[b + 1]; t++)
            for (size_t j = 0; j < l; j++) {
                const Fr x = fr_pow(w, cell[t] + m * j);
                Fr acc = fr_zero();
                for (size_t i = d; i-- > 0;) acc = fr_add(fr_mul(acc, x), c[i]);
                memcpy(&values[4 * (t * l + j)], acc.d, 32);
            }
    }
    if (alter) {
        Fr v;
        memcpy(v.d, &values[4 * (size_t)off[1] * l], 32);
        v = fr_add(v, fr_one());
        memcpy(&values[4 * (size_t)off[1] * l], v.d, 32);
    }
    const std::vector<uint64_t> values_kept = values;
    std::vector<uint64_t> out((size_t)batch * stride * 4, FILL), vals((size_t)batch * n * 4, FILL), first((size_t)batch, FILL);
    bbgpu_kzg_recover_each_report rep;
    memset(&rep, 0xEE, sizeof rep);
    KzgRecoverEachShape S;
    char why[320] = "";
    int rc = kzg_recover_each_verdict("test", off.data(), cell.data(), values.data(), n, l, d, batch, out.data(), stride, &rep, &S, why, sizeof why);
    size_t most = 0;
    for (size_t v : mu) most = v > most ? v : most;
    CHECK(rc == BBGPU_OK && S.m == m && S.max_missing == most && S.total == cell.size(), "%s: verdict %d %s", what, rc, why);
    if (rc) return;
    rc = kzg_recover_cells_each_host(S, off.data(), cell.data(), values.data(), d, batch, out.data(), stride, vals.data(), first.data(), &rep, why, sizeof why);
    CHECK(rc == BBGPU_OK, "%s: %d %s", what, rc, why);
    CHECK(values == values_kept, "%s: the values were written to", what);
    const size_t present1 = (size_t)(off[2] - off[1]) * l;
    const bool seen = alter && present1 > d;
    CHECK(rep.max_missing == most && rep.consistent == (seen ? 0u : 1u) && rep.first_bad_poly == (seen ? 1u : 0u) &&
              (seen ? rep.first_bad_coeff >= d && rep.first_bad_coeff < present1 && first[1] == rep.first_bad_coeff : rep.first_bad_coeff == 0 && first[1] == ~0ull),
          "%s: report %u %u %llu %llu", what, rep.consistent, rep.first_bad_poly, (unsigned long long)rep.first_bad_coeff, (unsigned long long)rep.max_missing);
    for (int b = 0; b < batch; b++) {
        if (b != 1) CHECK(first[b] == ~0ull, "%s: first_bad of polynomial %d", what, b);
        if (b != 1 || !alter) CHECK(!memcmp(&out[(size_t)b * stride * 4], &coeffs[(size_t)b * n], n * 32), "%s: polynomial %d", what, b);
        for (size_t i = 4 * n; i < 4 * stride; i++) CHECK(out[(size_t)b * stride * 4 + i] == FILL, "%s: padding of polynomial %d written", what, b);
        if (b != 1 || !alter)
            for (size_t t = off[b]; t < off[b + 1]; t++) // the transform holds the listed values again
                for (size_t j = 0; j < l; j++)
                    CHECK(!memcmp(&vals[4 * ((size_t)b * n + cell[t] + m * j)], &values[4 * (t * l + j)], 32), "%s: value (%d, %zu, %zu)", what, b, t, j);
    }
}

static void refused(size_t n, size_t l, size_t d, const std::vector<uint32_t>& off, const std::vector<uint32_t>& cell, size_t stride, int want, const char* text,
                    const char* what)
{
    const int batch = (int)off.size() - 1;
    std::vector<uint64_t> values((cell.size() + 1) * (l ? l : 1) * 4, 0), out(64, FILL);
    bbgpu_kzg_recover_each_report rep;
    KzgRecoverEachShape S;
    char why[320] = "";
    const int rc = kzg_recover_each_verdict("test", off.data(), cell.data(), values.data(), n, l, d, batch, out.data(), stride, &rep, &S, why, sizeof why);
    CHECK(rc == want && strstr(why, text), "%s: %d, want %d (%s)", what, rc, want, why);
    for (uint64_t v : out) CHECK(v == FILL, "%s: output written", what);
}

int main()
{
    const size_t sizes[2][2] = { { 16, 4 }, { 64, 1 } };
    for (const auto& s : sizes) {
        const size_t n = s[0], l = s[1], m = n / l, d = n / 2;
        run(n, l, d, { 0, 1, m / 2 }, n + 5, false, "none, one, as many as d allows");
        run(n, l, 1, { m - 1, 0, 1 }, n, false, "a constant from one cell beside full lists");
        run(n, l, d, { m / 2, 1, 0 }, n + 5, true, "one altered value in polynomial 1, redundant cells");
        run(n, l, d, { 0, m / 2, 1 }, n, true, "one altered value in polynomial 1, no redundancy");
    }
    refused(12, 4, 4, { 0, 2 }, { 0, 1 }, 12, BBGPU_ERR_SIZE, "power of two", "n not a power of two");
    refused(256, 128, 4, { 0, 2 }, { 0, 1 }, 256, BBGPU_ERR_SIZE, "power of two", "coset above 64");
    refused(16, 16, 4, { 0, 1 }, { 0 }, 16, BBGPU_ERR_SIZE, "at least 2", "one cell per polynomial");
    refused(16, 4, 0, { 0, 2 }, { 0, 1 }, 16, BBGPU_ERR_SIZE, "degree bound 0", "degree bound 0");
    refused(16, 4, 17, { 0, 4 }, { 0, 1, 2, 3 }, 16, BBGPU_ERR_SIZE, "degree bound 17", "degree bound above n");
    refused(16, 4, 4, { 0 }, {}, 16, BBGPU_ERR_SIZE, "batch 0", "batch 0");
    refused(16, 4, 4, { 0, 2 }, { 0, 1 }, 15, BBGPU_ERR_SIZE, "stride 15", "stride below n");
    refused(16, 4, 9, { 0, 3, 5 }, { 0, 1, 2, 0, 1 }, 16, BBGPU_ERR_SIZE, "polynomial 1 lists 2", "too few cells in polynomial 1");
    refused(16, 4, 4, { 0, 2, 2 }, { 0, 1 }, 16, BBGPU_ERR_SIZE, "polynomial 1 lists 0", "no cell in polynomial 1");
    refused(16, 4, 4, { 0, 2, 7 }, { 0, 1, 0, 1, 2, 3, 0 }, 16, BBGPU_ERR_SIZE, "polynomial 1 lists 5", "more cells than there are");
    refused(16, 4, 4, { 1, 2 }, { 0, 1 }, 16, BBGPU_ERR_ARG, "cell_offsets[0] = 1", "offsets that do not start at 0");
    refused(16, 4, 4, { 0, 2, 1 }, { 0, 1 }, 16, BBGPU_ERR_ARG, "polynomial 1: cell_offsets[2] = 1", "offsets that decrease");
    refused(16, 4, 4, { 0, 2, 4 }, { 0, 1, 0, 4 }, 16, BBGPU_ERR_ARG, "polynomial 1: cell[3] = 4", "a cell that does not exist");
    refused(16, 4, 4, { 0, 2, 5 }, { 0, 1, 2, 0, 2 }, 16, BBGPU_ERR_ARG, "polynomial 1: cell[4] = 2 (position 2 of its list) is listed twice", "a cell listed twice");
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
