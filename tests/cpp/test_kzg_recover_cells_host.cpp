// The host twin of bbgpu_kzg_recover_cells (csrc/host_kzg_recover_cells.hpp: kzg_recover_verdict, kzg_recover_cells_host) under AddressSanitizer and
// UndefinedBehaviorSanitizer, at (n, l) = (8, 1), (16, 4) and (256, 64).  The expected coefficients are those of the polynomial the cells were made from
// (values by Horner's rule, never a transform); batch 1 and 3, with padding between the polynomials that must stay as it was; no cell missing, one, and as
// many as the degree bound allows; cells listed in reverse order; one altered value with and without redundancy; refused calls, which write nothing.
// A stand-alone program with its own main; built and run by tests/test_kzg_recover_cells_host.py::test_host_twin_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_kzg_recover_cells.hpp"

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

// alter: -1 none, else the index of the value of polynomial 0 that gets one added
static void run(size_t n, size_t l, size_t d, size_t mu, int batch, size_t stride, long alter, const char* what)
{
    const size_t m = n / l, count = m - mu, present = count * l;
    int log2n = 0;
    while (((size_t)1 << log2n) < n) log2n++;
    const Fr w = fr_root_of_unity(log2n);
    std::vector<bool> gone(m, false); // every other cell from 0 while that gives mu of them, else the first mu
    for (size_t i = 0; i < mu; i++) gone[mu <= m / 2 ? 2 * i : i] = true;
    std::vector<uint32_t> cell; // listed from the top
    for (size_t k = m; k-- > 0;)
        if (!gone[k]) cell.push_back((uint32_t)k);
    CHECK(cell.size() == count, "%s: cell list", what);
    std::vector<Fr> coeffs((size_t)batch * n, fr_zero());
    std::vector<uint64_t> values((size_t)batch * present * 4);
    for (int b = 0; b < batch; b++) {
        Fr* c = &coeffs[(size_t)b * n];
        for (size_t i = 0; i < d; i++) c[i] = random_fr();
        for (size_t t = 0; t < count; t++)
            for (size_t j = 0; j < l; j++) {
                const Fr x = fr_pow(w, cell[t] + m * j);
                Fr acc = fr_zero();
                for (size_t i = d; i-- > 0;) acc = fr_add(fr_mul(acc, x), c[i]);
                memcpy(&values[4 * (((size_t)b * count + t) * l + j)], acc.d, 32);
            }
    }
    if (alter >= 0) {
        Fr v;
        memcpy(v.d, &values[4 * (size_t)alter], 32);
        v = fr_add(v, fr_one());
        memcpy(&values[4 * (size_t)alter], v.d, 32);
    }
    const std::vector<uint64_t> values_kept = values;
    std::vector<uint64_t> out((size_t)batch * stride * 4, FILL), vals((size_t)batch * n * 4, FILL);
    bbgpu_kzg_recover_report rep;
    memset(&rep, 0xEE, sizeof rep);
    KzgRecoverShape S;
    char why[320] = "";
    int rc = kzg_recover_verdict("test", cell.data(), count, values.data(), n, l, d, batch, out.data(), stride, &rep, &S, why, sizeof why);
    CHECK(rc == BBGPU_OK && S.m == m && S.mu == mu && S.missing.size() == mu, "%s: verdict %d %s", what, rc, why);
    if (rc) return;
    rc = kzg_recover_cells_host(S, cell.data(), count, values.data(), d, batch, out.data(), stride, vals.data(), &rep, why, sizeof why);
    CHECK(rc == BBGPU_OK, "%s: %d %s", what, rc, why);
    CHECK(values == values_kept, "%s: the values were written to", what);
    const bool seen = alter >= 0 && present > d;
    CHECK(rep.missing == mu && rep.consistent == (seen ? 0u : 1u) && rep.first_bad_poly == 0 && (seen ? rep.first_bad_coeff >= d && rep.first_bad_coeff < present
                                                                                                   : rep.first_bad_coeff == 0),
          "%s: report %u %u %llu %llu", what, rep.consistent, rep.first_bad_poly, (unsigned long long)rep.first_bad_coeff, (unsigned long long)rep.missing);
    for (int b = 0; b < batch; b++) {
        if (b > 0 || alter < 0) CHECK(!memcmp(&out[(size_t)b * stride * 4], &coeffs[(size_t)b * n], n * 32), "%s: polynomial %d", what, b);
        for (size_t i = 4 * n; i < 4 * stride; i++) CHECK(out[(size_t)b * stride * 4 + i] == FILL, "%s: padding of polynomial %d written", what, b);
        if (b > 0 || alter < 0)
            for (size_t t = 0; t < count; t++) // the transform holds the listed values again
                for (size_t j = 0; j < l; j++)
                    CHECK(!memcmp(&vals[4 * ((size_t)b * n + cell[t] + m * j)], &values[4 * (((size_t)b * count + t) * l + j)], 32), "%s: value (%d, %zu, %zu)", what, b,
                          t, j);
    }
}

static void refused(size_t n, size_t l, size_t d, const std::vector<uint32_t>& cell, int batch, size_t stride, int want, const char* what)
{
    std::vector<uint64_t> values((size_t)(batch > 0 ? batch : 1) * cell.size() * (l ? l : 1) * 4, 0), out(64, FILL);
    bbgpu_kzg_recover_report rep;
    KzgRecoverShape S;
    char why[320] = "";
    const int rc = kzg_recover_verdict("test", cell.data(), cell.size(), values.data(), n, l, d, batch, out.data(), stride, &rep, &S, why, sizeof why);
    CHECK(rc == want && why[0], "%s: %d, want %d (%s)", what, rc, want, why);
}

int main()
{
    const size_t sizes[3][2] = { { 8, 1 }, { 16, 4 }, { 256, 64 } };
    for (const auto& s : sizes) {
        const size_t n = s[0], l = s[1], m = n / l, d = n / 2;
        run(n, l, d, 0, 1, n, -1, "no cell missing");
        run(n, l, d, 1, 3, n + 5, -1, "one cell missing, padded");
        run(n, l, d, m / 2, 1, n, -1, "as many missing as d allows");
        run(n, l, 1, m - 1, 3, n + 5, -1, "a constant from one cell");
        run(n, l, n, 0, 1, n, -1, "full degree");
        run(n, l, d, 1, 3, n + 5, 0, "one altered value, redundant cells");
        run(n, l, d, m / 2, 1, n, (long)(d - 1), "one altered value, no redundancy");
    }
    refused(12, 4, 4, { 0, 1 }, 1, 12, BBGPU_ERR_SIZE, "n not a power of two");
    refused(16, 3, 4, { 0, 1 }, 1, 16, BBGPU_ERR_SIZE, "coset not a power of two");
    refused(256, 128, 4, { 0, 1 }, 1, 256, BBGPU_ERR_SIZE, "coset above 64");
    refused(16, 16, 4, { 0 }, 1, 16, BBGPU_ERR_SIZE, "one cell per polynomial");
    refused((size_t)1 << 17, 1, 2, { 0, 1 }, 1, (size_t)1 << 17, BBGPU_ERR_SIZE, "more than 2^16 cells");
    refused(16, 4, 0, { 0, 1 }, 1, 16, BBGPU_ERR_SIZE, "degree bound 0");
    refused(16, 4, 17, { 0, 1, 2, 3 }, 1, 16, BBGPU_ERR_SIZE, "degree bound above n");
    refused(16, 4, 9, { 0, 1 }, 1, 16, BBGPU_ERR_SIZE, "too few cells");
    refused(16, 4, 4, { 0, 1, 2, 3, 0 }, 1, 16, BBGPU_ERR_SIZE, "more cells than there are");
    refused(16, 4, 4, { 0, 1 }, 0, 16, BBGPU_ERR_SIZE, "batch 0");
    refused(16, 4, 4, { 0, 1 }, 65, 16, BBGPU_ERR_SIZE, "batch 65");
    refused(16, 4, 4, { 0, 1 }, 1, 15, BBGPU_ERR_SIZE, "stride below n");
    refused(16, 4, 4, { 0, 4 }, 1, 16, BBGPU_ERR_ARG, "a cell that does not exist");
    refused(16, 4, 4, { 2, 0, 2 }, 1, 16, BBGPU_ERR_ARG, "a cell listed twice");
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
