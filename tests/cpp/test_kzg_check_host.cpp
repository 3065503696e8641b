// Host twins of the batched check of KZG openings (csrc/host_kzg_check_batch.hpp: kzg_check_host behind its argument checks) under AddressSanitizer and
// UndefinedBehaviorSanitizer.  The program makes its own string P_j = x^j G and x G2 from a secret, commits to polynomials with the host bucket
// method, opens them with kate_opening at points on and off the domain, and holds the twins to: the verdict of the 64-claim check the library had
// before (kzg_check_openings below), the shared layout against the per-claim layout, the open-all form against explicit z = omega^i, infinities, findings,
// and the bisection.
// A stand-alone program with its own main; built and run by tests/test_kzg_check_host.py::test_host_twins_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_g2.hpp"
#include "../../barretenberg_amd/csrc/host_kzg_check_batch.hpp"

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

struct Point {
    uint64_t w[8];
};
static const Point INF = { { 0, 0, 0, 0, 0, 0, 0, 1ULL << 63 } };
static Point normalised(const Xyzz& p)
{
    uint64_t o[12];
    g1_to_normalised(p, o);
    Point r;
    memcpy(r.w, o, 64);
    return r;
}

struct World {
    size_t n;
    int log2n;
    std::vector<Point> rows;            // P_j = x^j G
    uint64_t g2_x[16];
    std::vector<std::vector<Fr>> coeffs; // polynomial 1 is constant
    std::vector<Point> commitments;
};
static Point commit(const World& W, const std::vector<Fr>& c) { return normalised(msm_pippenger(c[0].d, W.rows[0].w, W.n, 8)); }
static World make_world(size_t n, int log2n, int batch)
{
    World W;
    W.n = n;
    W.log2n = log2n;
    const Fr x = fr_mul(random_fr(), fr_one());
    Point g;
    const Fq gy = fq_dbl(FQ_ONE);
    memcpy(g.w, FQ_ONE.d, 32);
    memcpy(g.w + 4, gy.d, 32);
    Fr pw = fr_one();
    for (size_t j = 0; j < n; j++) {
        W.rows.push_back(normalised(msm_small(pw.d, g.w, 1, 8)));
        pw = fr_mul(pw, x);
    }
    G2Affine xg2;
    if (!g2_scalar_mul_affine(G2_ONE, x, &xg2)) CHECK(false, "x G2");
    memcpy(W.g2_x, &xg2, 128);
    for (int b = 0; b < batch; b++) {
        std::vector<Fr> c(n);
        for (size_t j = 0; j < n; j++) c[j] = (b == 1 && j > 0) ? fr_zero() : random_fr();
        W.coeffs.push_back(c);
        W.commitments.push_back(commit(W, c));
    }
    return W;
}
// the claim (z, y, pi) of polynomial b at z
static void open_at(const World& W, int b, const Fr& z, Fr* y, Point* pi)
{
    std::vector<Fr> q(W.n);
    *y = kate_opening(W.coeffs[b][0].d, q[0].d, W.n, z);
    *pi = normalised(msm_pippenger(q[0].d, W.rows[0].w, W.n, 8));
}

struct Claims {
    std::vector<uint32_t> which;
    std::vector<Fr> z, y;
    std::vector<Point> pi, expanded;
};
static bbgpu_kzg_check_report run(const World& W, const Claims& C, bool shared, const uint64_t seed[4], int flags)
{
    KzgCheckCall K;
    K.commitments = shared ? W.commitments[0].w : C.expanded[0].w;
    K.which = shared ? C.which.data() : nullptr;
    K.S = shared ? W.commitments.size() : 0;
    K.z = C.z[0].d;
    K.y = C.y[0].d;
    K.proofs = C.pi[0].w;
    K.count = C.z.size();
    bbgpu_kzg_check_report R;
    const char* why = "";
    CHECK(kzg_check_args(K, !shared, W.commitments.size(), W.g2_x, flags, &R, &why) == BBGPU_OK, "arguments: %s", why);
    CHECK(kzg_check_host(K, W.g2_x, seed, flags, &R) == BBGPU_OK, "the check ran");
    return R;
}
// The definition claim by claim, as the 64-claim entry computed it before it became a call of the twin: plain tables, points at infinity left out (the
// twin gives them a zero scalar).  Kept here as the twin's independent check.
static bool kzg_check_openings(const uint64_t* commitments, const uint64_t* z, const uint64_t* y, const uint64_t* proofs, size_t k, const uint64_t g2_x[16],
                               const uint64_t seed[4])
{
    std::vector<uint64_t> pa, sa, pb, sb;
    auto push = [](std::vector<uint64_t>& pts, std::vector<uint64_t>& sc, const uint64_t* p, const Fr& s) {
        if (g1_words_is_inf(p)) return;
        Fq c[2];
        g1_words_canonical(p, &c[0], &c[1]);
        pts.insert(pts.end(), c[0].d, c[0].d + 4);
        pts.insert(pts.end(), c[1].d, c[1].d + 4);
        sc.insert(sc.end(), s.d, s.d + 4);
    };
    Fr ysum = fr_zero();
    for (size_t t = 0; t < k; t++) {
        Fr rho, zt, yt;
        srs_check_rho(seed, t, rho.d);
        memcpy(zt.d, z + 4 * t, 32);
        memcpy(yt.d, y + 4 * t, 32);
        push(pa, sa, commitments + 8 * t, rho);
        push(pa, sa, proofs + 8 * t, fr_mul(rho, zt));
        push(pb, sb, proofs + 8 * t, rho);
        ysum = fr_add(ysum, fr_mul(rho, yt));
    }
    uint64_t g[8], a12[12], b12[12];
    g1_generator_words(g);
    push(pa, sa, g, fr_neg(ysum));
    g1_to_normalised(msm_pippenger(sa.data(), pa.data(), sa.size() / 4, 8), a12);
    g1_to_normalised(msm_pippenger(sb.data(), pb.data(), sb.size() / 4, 8), b12);
    return pair_is_one(a12, b12, &G2_ONE, g2_x);
}
static bool same(const bbgpu_kzg_check_report& a, const bbgpu_kzg_check_report& b)
{
    return a.count == b.count && a.bad_points == b.bad_points && a.first_bad == b.first_bad && a.first_bad_is_proof == b.first_bad_is_proof && a.g2_ok == b.g2_ok &&
           a.ok == b.ok && a.rounds == b.rounds && a.first_failing == b.first_failing && !memcmp(a.seed, b.seed, 32) && !memcmp(a.a, b.a, 64) && !memcmp(a.b, b.b, 64);
}

int main()
{
    const uint64_t seed[4] = { 0x0123456789ABCDEFULL, 0xFEDCBA9876543210ULL, 0x0F1E2D3C4B5A6978ULL, 0x1122334455667788ULL };
    const size_t n = 8;
    const int batch = 3;
    const World W = make_world(n, 3, batch);
    const Fr omega = fr_root_of_unity(3);
    CHECK(g1_words_is_inf(commit(W, std::vector<Fr>(n, fr_zero())).w), "the zero polynomial commits to infinity");

    // 40 claims: polynomials in turn, points on the domain and off it, z and y also as representatives that are not canonical
    Claims C;
    for (size_t t = 0; t < 40; t++) {
        const int b = (int)(t % batch);
        const Fr z = t % 4 == 3 ? random_fr() : fr_pow(omega, t % n);
        Fr y;
        Point pi;
        open_at(W, b, z, &y, &pi);
        if (b == 1) CHECK(g1_words_is_inf(pi.w), "the proof of a constant is at infinity");
        C.which.push_back((uint32_t)b);
        C.z.push_back(z);
        C.y.push_back(y);
        C.pi.push_back(pi);
        C.expanded.push_back(W.commitments[b]);
    }
    const bbgpu_kzg_check_report honest = run(W, C, false, seed, 0);
    CHECK(honest.ok == 1 && honest.rounds == 1 && honest.bad_points == 0 && honest.first_failing == -1 && honest.count == 40, "honest claims");
    CHECK(kzg_check_openings(C.expanded[0].w, C.z[0].d, C.y[0].d, C.pi[0].w, 40, W.g2_x, seed), "the 64-claim check accepts them");
    CHECK(same(honest, run(W, C, true, seed, 0)), "shared layout against per-claim layout");
    CHECK(same(honest, run(W, C, true, seed, BBGPU_KZG_CHECK_LOCATE)), "nothing to locate");

    for (size_t t : { (size_t)0, (size_t)20, (size_t)39 }) { // a false value, a wrong proof: both checks refuse, the bisection names the claim
        for (int what = 0; what < 2; what++) {
            Claims T = C;
            if (what == 0) T.y[t] = fr_add(fr_mul(T.y[t], fr_one()), fr_one());
            else T.pi[t] = W.rows[1 + t % 3];
            CHECK(!kzg_check_openings(T.expanded[0].w, T.z[0].d, T.y[0].d, T.pi[0].w, 40, W.g2_x, seed), "the 64-claim check refuses claim %zu", t);
            for (bool shared : { false, true }) {
                const bbgpu_kzg_check_report R = run(W, T, shared, seed, BBGPU_KZG_CHECK_LOCATE);
                CHECK(R.ok == 0 && R.first_failing == (int64_t)t && R.rounds >= 1 && R.rounds <= 7, "claim %zu located (%lld, %u rounds)", t, (long long)R.first_failing, R.rounds);
                const bbgpu_kzg_check_report Q = run(W, T, shared, seed, 0);
                CHECK(Q.ok == 0 && Q.first_failing == -1 && Q.rounds == 1, "claim %zu without the flag", t);
            }
        }
    }
    { // findings: a proof and a commitment off the curve
        Claims T = C;
        T.pi[6].w[4] ^= 1; // claim 6 is of polynomial 0: a finite proof
        T.pi[33].w[0] ^= 1;
        bbgpu_kzg_check_report R = run(W, T, true, seed, BBGPU_KZG_CHECK_LOCATE);
        CHECK(R.ok == 0 && R.rounds == 0 && R.bad_points == 2 && R.first_bad == 6 && R.first_bad_is_proof == 1 && R.a[7] == 1ULL << 63, "two proofs off the curve");
        T.expanded[6].w[4] ^= 1;
        R = run(W, T, false, seed, 0);
        CHECK(R.ok == 0 && R.bad_points == 3 && R.first_bad == 6 && R.first_bad_is_proof == 0, "C_6 before pi_6");
        World V = W;
        V.commitments[2].w[0] ^= 1;
        R = run(V, T, true, seed, 0);
        CHECK(R.ok == 0 && R.bad_points == 3 && R.first_bad == 2 && R.first_bad_is_proof == 0, "a shared commitment before every claim");
    }
    { // the open-all form against explicit z = omega^i, with padded values
        const size_t stride = n + 3;
        std::vector<Fr> values(batch * stride, fr_from_u64(0x5A5A));
        std::vector<Point> proofs(batch * n);
        Claims E;
        for (int b = 0; b < batch; b++)
            for (size_t i = 0; i < n; i++) {
                Fr y;
                open_at(W, b, fr_pow(omega, i), &y, &proofs[b * n + i]);
                values[b * stride + i] = y;
                E.which.push_back((uint32_t)b);
                E.z.push_back(fr_pow(omega, i));
                E.y.push_back(y);
                E.pi.push_back(proofs[b * n + i]);
            }
        KzgCheckCall K;
        K.commitments = W.commitments[0].w;
        K.S = (size_t)batch;
        K.y = values[0].d;
        K.y_stride = stride;
        K.proofs = proofs[0].w;
        K.count = batch * n;
        K.open_all = true;
        CHECK(kzg_check_open_all_sizes_ok(n, stride, batch, &K.log2n) && K.log2n == 3, "sizes");
        bbgpu_kzg_check_report R;
        CHECK(kzg_check_host(K, W.g2_x, seed, 0, &R) == BBGPU_OK && R.ok == 1, "open-all form");
        CHECK(same(R, run(W, E, true, seed, 0)), "open-all form against the shared layout");
        values[2 * stride + n - 1] = fr_add(fr_mul(values[2 * stride + n - 1], fr_one()), fr_one());
        CHECK(kzg_check_host(K, W.g2_x, seed, BBGPU_KZG_CHECK_LOCATE, &R) == BBGPU_OK && R.ok == 0 && R.first_failing == (int64_t)(batch * n - 1), "the last value");
        int lg;
        CHECK(!kzg_check_open_all_sizes_ok(0, 8, 1, &lg) && !kzg_check_open_all_sizes_ok(12, 12, 1, &lg) && !kzg_check_open_all_sizes_ok(8, 7, 1, &lg) &&
                  !kzg_check_open_all_sizes_ok(8, 8, 0, &lg) && !kzg_check_open_all_sizes_ok(8, 8, 65, &lg) &&
                  !kzg_check_open_all_sizes_ok((size_t)1 << 20, (size_t)1 << 20, 2, &lg) && kzg_check_open_all_sizes_ok((size_t)1 << 20, (size_t)1 << 20, 1, &lg) &&
                  kzg_check_open_all_sizes_ok(1, 1, 64, &lg) && lg == 0,
              "sizes of the open-all form");
    }
    { // one claim; every proof at infinity (B is the point at infinity); a commitment at infinity with the claim 0 = 0
        Claims one;
        one.which = { 0 };
        one.z = { C.z[3] };
        one.y = { C.y[3] };
        one.pi = { C.pi[3] };
        one.expanded = { C.expanded[3] };
        CHECK(run(W, one, false, seed, 0).ok == 1 && run(W, one, true, seed, BBGPU_KZG_CHECK_LOCATE).ok == 1, "one claim");
        Claims K;
        for (size_t t = 1; t < 40; t += 3) {
            K.which.push_back(1);
            K.z.push_back(C.z[t]);
            K.y.push_back(C.y[t]);
            K.pi.push_back(C.pi[t]);
            K.expanded.push_back(C.expanded[t]);
        }
        const bbgpu_kzg_check_report R = run(W, K, true, seed, 0);
        CHECK(R.ok == 1 && R.b[7] == 1ULL << 63 && same(R, run(W, K, false, seed, 0)), "proofs at infinity");
        World Z = W;
        Z.commitments[1] = INF;
        Claims zero;
        zero.which = { 0, 1 };
        zero.z = { C.z[0], random_fr() };
        zero.y = { C.y[0], fr_zero() };
        zero.pi = { C.pi[0], INF };
        zero.expanded = { W.commitments[0], INF };
        CHECK(run(Z, zero, true, seed, 0).ok == 1 && run(Z, zero, false, seed, 0).ok == 1, "the zero polynomial");
        zero.y[1] = fr_one();
        CHECK(run(Z, zero, true, seed, 0).ok == 0 && run(Z, zero, false, seed, 0).ok == 0, "the zero polynomial does not take the value one");
    }
    { // the argument verdicts
        KzgCheckCall K;
        bbgpu_kzg_check_report R;
        const char* why = "";
        K.commitments = W.commitments[0].w;
        K.which = C.which.data();
        K.S = 2; // labels reach 2
        K.z = C.z[0].d;
        K.y = C.y[0].d;
        K.proofs = C.pi[0].w;
        K.count = 40;
        CHECK(kzg_check_args(K, false, 2, W.g2_x, 0, &R, &why) == BBGPU_ERR_ARG, "a label out of range");
        CHECK(kzg_check_args(K, false, 3, W.g2_x, 2, &R, &why) == BBGPU_ERR_ARG && kzg_check_args(K, false, 65, W.g2_x, 0, &R, &why) == BBGPU_ERR_ARG, "flags, commitments");
        K.count = 0;
        CHECK(kzg_check_args(K, false, 3, W.g2_x, 0, &R, &why) == BBGPU_ERR_SIZE, "no claims");
        K.count = 40;
        uint64_t bad[16];
        memcpy(bad, W.g2_x, 128);
        bad[0] ^= 1;
        CHECK(kzg_check_args(K, false, 3, bad, 0, &R, &why) == BBGPU_ERR_ARG && kzg_check_args(K, false, 3, nullptr, 0, &R, &why) == BBGPU_ERR_ARG, "g2_x");
        CHECK(kzg_check_args(K, false, 3, W.g2_x, 0, &R, &why) == BBGPU_OK, "a good call");
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
