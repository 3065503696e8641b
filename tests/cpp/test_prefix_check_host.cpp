// csrc/host_random_check.hpp, prefix_check (host PRODUCT code: the verdict and the bisection every random-combination check ends in) compiled with
// -fsanitize=address,undefined and driven with fake sums and a fake relation: sums(m) records m and answers a12[0] = b12[0] = m, accept is m <= f, so that
// prefixes up to f pass and item f is the first to fail.  Built and run by tests/test_prefix_check_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_random_check.hpp"

using namespace bbgpu::host;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); fails++; } } while (0)

static uint32_t ceil_log2(size_t n)
{
    uint32_t k = 0;
    while (((size_t)1 << k) < n) k++;
    return k;
}

// One run: items [0, f) are good, f == count: nothing fails.  fail_at: the call of sums (from 1) that returns -7; 0: none does.
struct Run {
    std::vector<size_t> seen;
    PrefixVerdict v;
    int rc;
};
static Run run(size_t count, size_t f, bool locate, size_t fail_at = 0)
{
    Run r;
    memset(&r.v, 0xA5, sizeof r.v);
    r.rc = prefix_check(
        count, locate,
        [&](size_t m, uint64_t* a12, uint64_t* b12) {
            r.seen.push_back(m);
            if (r.seen.size() == fail_at) return -7;
            for (int i = 0; i < 12; i++) a12[i] = b12[i] = m + (uint64_t)i;
            return 0;
        },
        [&](const uint64_t* a12, const uint64_t* b12) { return a12[0] == b12[0] && a12[0] <= f; }, &r.v);
    return r;
}
static bool kept_first_round(const PrefixVerdict& v, size_t count)
{
    for (int i = 0; i < 12; i++)
        if (v.a[i] != count + (uint64_t)i || v.b[i] != count + (uint64_t)i) return false;
    return true;
}

static void check_case(size_t count, size_t f)
{
    const bool good = f == count;
    const Run r = run(count, f, true);
    CHECK(r.rc == 0, "count %zu f %zu: rc %d", count, f, r.rc);
    CHECK(r.v.ok == good, "count %zu f %zu: ok %d", count, f, (int)r.v.ok);
    CHECK(r.v.first_failing == (good ? SIZE_MAX : f), "count %zu f %zu: first_failing %zu", count, f, r.v.first_failing);
    CHECK(r.v.rounds == r.seen.size(), "count %zu f %zu: rounds %u, %zu calls", count, f, r.v.rounds, r.seen.size());
    CHECK(r.v.rounds <= 1 + ceil_log2(count), "count %zu f %zu: %u rounds, at most %u", count, f, r.v.rounds, 1 + ceil_log2(count));
    CHECK(good ? r.seen.size() == 1 : true, "count %zu: a passing check took %zu rounds", count, r.seen.size());
    CHECK(!r.seen.empty() && r.seen[0] == count, "count %zu f %zu: the first round is not over the whole input", count, f);
    for (size_t m : r.seen) CHECK(m >= 1 && m <= count, "count %zu f %zu: a round over %zu items", count, f, m);
    CHECK(kept_first_round(r.v, count), "count %zu f %zu: a / b kept are not the first round's (a[0] = %llu)", count, f, (unsigned long long)r.v.a[0]);

    const Run q = run(count, f, false);
    CHECK(q.rc == 0 && q.seen.size() == 1 && q.seen[0] == count && q.v.rounds == 1, "count %zu f %zu without LOCATE: %zu calls", count, f, q.seen.size());
    CHECK(q.v.ok == good && q.v.first_failing == SIZE_MAX, "count %zu f %zu without LOCATE: ok %d first_failing %zu", count, f, (int)q.v.ok, q.v.first_failing);
    CHECK(kept_first_round(q.v, count), "count %zu f %zu without LOCATE: a / b", count, f);
}

int main()
{
    for (size_t count = 1; count <= 9; count++)
        for (size_t f = 0; f <= count; f++) check_case(count, f);
    for (size_t f = 0; f <= 1000; f++) check_case(1000, f);

    // one failing item is found in the one round
    {
        const Run r = run(1, 0, true);
        CHECK(r.rc == 0 && !r.v.ok && r.v.first_failing == 0 && r.v.rounds == 1 && r.seen.size() == 1, "count 1: first_failing %zu after %u rounds", r.v.first_failing,
              r.v.rounds);
    }
    // an error from sums ends the check at once; what the first round found stays
    {
        const size_t clean = run(8, 2, true).seen.size();
        CHECK(clean == 4, "count 8 f 2 takes %zu rounds", clean);
        for (size_t k = 1; k <= 4; k++) {
            const Run r = run(8, 2, true, k);
            CHECK(r.rc == -7, "error in call %zu: rc %d", k, r.rc);
            CHECK(r.seen.size() == k, "error in call %zu: %zu calls", k, r.seen.size());
            CHECK(r.v.rounds == k - 1, "error in call %zu: rounds %u", k, r.v.rounds);
            CHECK(r.v.first_failing == SIZE_MAX, "error in call %zu: first_failing %zu", k, r.v.first_failing);
            if (k > 1) CHECK(kept_first_round(r.v, 8) && !r.v.ok, "error in call %zu: the first round's a / b / ok are gone", k);
        }
    }
    if (fails) {
        printf("%d FAILED\n", fails);
        return 1;
    }
    printf("ALL OK\n");
    return 0;
}
