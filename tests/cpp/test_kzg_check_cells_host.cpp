// Host twins of the check of KZG cell proofs (csrc/host_kzg_check_cells.hpp: kzg_cells_host behind its argument checks, kzg_cells_key_ok) under
// AddressSanitizer and UndefinedBehaviorSanitizer.  The program makes its own string P_j = x^j G, x G2 and [x^l] G2 from a secret, commits to polynomials
// with the host bucket method, makes the cell proofs by the quotient definition (synthetic division by X^l - psi^k) and the values by Horner's rule, and
// holds the twins at l = 4 and l = 64 to: the definition cell by cell with r_k = f mod (X^l - psi^k) reduced term by term (no transform), the labelled
// form against the open-cosets form, infinities, findings, the key check, the argument verdicts and the bisection.
// A stand-alone program with its own main; built and run by tests/test_kzg_check_cells_host.py::test_host_twin_under_sanitizers.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/host_g2.hpp"
#include "../../barretenberg_amd/csrc/host_kzg_check_cells.hpp"

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
    size_t n, l, m;
    int log2n;
    Fr omega, psi;
    std::vector<Point> rows; // P_j = x^j G
    uint64_t g2_x[16], g2_xl[16], g2_other[16];
    std::vector<std::vector<Fr>> coeffs; // polynomial 1 has degree < l
    std::vector<Point> commitments;
    std::vector<Fr> values;    // batch x n: the transforms, f_b(omega^i)
    std::vector<Point> proofs; // batch x m
};
static Point commit(const World& W, const std::vector<Fr>& c) { return normalised(msm_pippenger(c[0].d, W.rows[0].w, W.n, 8)); }
static void g2_of(const Fr& s, uint64_t out[16])
{
    G2Affine q;
    if (!g2_scalar_mul_affine(G2_ONE, s, &q)) CHECK(false, "a multiple of G2");
    memcpy(out, &q, 128);
}
static World make_world(size_t n, int log2n, size_t l, int batch)
{
    World W;
    W.n = n;
    W.l = l;
    W.m = n / l;
    W.log2n = log2n;
    W.omega = fr_root_of_unity(log2n);
    W.psi = fr_pow(W.omega, l);
    const Fr x = random_fr();
    Point g;
    g1_generator_words(g.w);
    Fr pw = fr_one();
    for (size_t j = 0; j < n; j++) {
        W.rows.push_back(normalised(msm_small(pw.d, g.w, 1, 8)));
        pw = fr_mul(pw, x);
    }
    g2_of(x, W.g2_x);
    g2_of(fr_pow(x, l), W.g2_xl);
    g2_of(fr_pow(x, l + 1), W.g2_other);
    for (int b = 0; b < batch; b++) {
        std::vector<Fr> c(n);
        for (size_t j = 0; j < n; j++) c[j] = (b == 1 && j >= l) ? fr_zero() : random_fr();
        W.coeffs.push_back(c);
        W.commitments.push_back(commit(W, c));
        for (size_t i = 0; i < n; i++) { // Horner at omega^i
            const Fr z = fr_pow(W.omega, i);
            Fr y = fr_zero();
            for (size_t j = n; j-- > 0;) y = fr_add(fr_mul(y, z), c[j]);
            W.values.push_back(y);
        }
        for (size_t k = 0; k < W.m; k++) { // q with f = q (X^l - z) + r: q_d = c_(d+l) + z q_(d+l)
            const Fr z = fr_pow(W.psi, k);
            std::vector<Fr> q(n, fr_zero());
            for (size_t d = n - l; d-- > 0;) q[d] = fr_add(c[d + l], d + l < n ? fr_mul(z, q[d + l]) : fr_zero());
            W.proofs.push_back(commit(W, q));
        }
    }
    return W;
}

struct Cells {
    std::vector<uint32_t> which, cell;
    std::vector<Fr> values; // count x l
    std::vector<Point> pi;
};
static void push_cell(const World& W, Cells& C, uint32_t b, uint32_t k)
{
    C.which.push_back(b);
    C.cell.push_back(k);
    for (size_t j = 0; j < W.l; j++) C.values.push_back(W.values[b * W.n + k + W.m * j]);
    C.pi.push_back(W.proofs[b * W.m + k]);
}
static KzgCellsCall labelled(const World& W, const Cells& C)
{
    KzgCellsCall K;
    K.commitments = W.commitments[0].w;
    K.S = W.commitments.size();
    K.which = C.which.data();
    K.cell = C.cell.data();
    K.values = C.values[0].d;
    K.proofs = C.pi[0].w;
    K.head = W.rows[0].w;
    K.count = C.pi.size();
    return K;
}
static bbgpu_kzg_check_report run(const World& W, KzgCellsCall K, int batch, const uint64_t* g2_xl, const uint64_t seed[4], int flags)
{
    bbgpu_kzg_check_report R;
    char why[160] = "";
    CHECK(kzg_cells_args(&K, W.n, W.l, batch, g2_xl, flags, &R, why, sizeof why) == BBGPU_OK, "arguments: %s", why);
    CHECK(kzg_cells_host(K, g2_xl, seed, flags, &R) == BBGPU_OK, "the check ran");
    return R;
}
// the definition for one cell: r_k = f mod (X^l - z) from the VALUES is what the twin computes; here it comes from the COEFFICIENTS, r_i = sum_d c_(i + d l) z^d
static bool cell_holds(const World& W, uint32_t b, uint32_t k, const Point& pi)
{
    const Fr z = fr_pow(W.psi, k);
    std::vector<uint64_t> pts, sc;
    auto push = [&](const Point& p, const Fr& s) {
        if (g1_words_is_inf(p.w)) return;
        pts.insert(pts.end(), p.w, p.w + 8);
        sc.insert(sc.end(), s.d, s.d + 4);
    };
    push(W.commitments[b], fr_one());
    for (size_t i = 0; i < W.l; i++) {
        Fr r = fr_zero(), zp = fr_one();
        for (size_t d = 0; i + d * W.l < W.n; d++) {
            r = fr_add(r, fr_mul(W.coeffs[b][i + d * W.l], zp));
            zp = fr_mul(zp, z);
        }
        push(W.rows[i], fr_neg(r));
    }
    push(pi, z);
    uint64_t a12[12], b12[12] = { 0 };
    if (sc.empty()) return g1_words_is_inf(pi.w);
    g1_to_normalised(msm_pippenger(sc.data(), pts.data(), sc.size() / 4, 8), a12);
    memcpy(b12, pi.w, 64);
    return pair_is_one(a12, b12, &G2_ONE, W.g2_xl);
}
static bool same(const bbgpu_kzg_check_report& a, const bbgpu_kzg_check_report& b)
{
    return a.count == b.count && a.bad_points == b.bad_points && a.first_bad == b.first_bad && a.first_bad_is_proof == b.first_bad_is_proof && a.g2_ok == b.g2_ok &&
           a.ok == b.ok && a.rounds == b.rounds && a.first_failing == b.first_failing && !memcmp(a.seed, b.seed, 32) && !memcmp(a.a, b.a, 64) && !memcmp(a.b, b.b, 64);
}

static void cases(size_t n, int log2n, size_t l)
{
    const uint64_t seed[4] = { 0x0123456789ABCDEFULL, 0xFEDCBA9876543210ULL, 0x0F1E2D3C4B5A6978ULL, 0x1122334455667788ULL };
    const int batch = 3;
    const World W = make_world(n, log2n, l, batch);
    const size_t m = W.m, all = batch * m;
    for (size_t k = 0; k < m; k++) CHECK(g1_words_is_inf(W.proofs[m + k].w), "degree < l: the proof of cell %zu is at infinity", k);
    for (uint32_t t = 0; t < all; t++) CHECK(cell_holds(W, t / m, t % m, W.proofs[t]), "l = %zu: cell %u holds by the definition", l, t);
    CHECK(!cell_holds(W, 0, 0, W.proofs[2 * m]), "the proof of another polynomial's cell does not"); // at m = 2 the cells of ONE polynomial share q

    // every cell once in the order of the open-cosets form, then some again in another order
    Cells C;
    for (uint32_t t = 0; t < all; t++) push_cell(W, C, t / m, t % m);
    KzgCellsCall O;
    O.commitments = W.commitments[0].w;
    O.values = W.values[0].d;
    O.proofs = W.proofs[0].w;
    O.head = W.rows[0].w;
    O.cosets = true;
    O.stride = n;
    const bbgpu_kzg_check_report honest = run(W, labelled(W, C), 0, W.g2_xl, seed, 0);
    CHECK(honest.ok == 1 && honest.rounds == 1 && honest.bad_points == 0 && honest.first_failing == -1 && honest.count == all, "l = %zu: honest cells", l);
    CHECK(same(honest, run(W, O, batch, W.g2_xl, seed, 0)), "the open-cosets form against the labelled form");
    CHECK(same(honest, run(W, O, batch, W.g2_xl, seed, BBGPU_KZG_CHECK_LOCATE)), "nothing to locate");
    { // padded transforms: the padding is not read
        const size_t stride = n + 3;
        std::vector<Fr> padded(batch * stride, fr_from_u64(0x5A5A));
        for (int b = 0; b < batch; b++)
            for (size_t i = 0; i < n; i++) padded[b * stride + i] = W.values[b * n + i];
        KzgCellsCall P = O;
        P.values = padded[0].d;
        P.stride = stride;
        CHECK(same(honest, run(W, P, batch, W.g2_xl, seed, 0)), "padded transforms");
    }
    Cells D = C;
    for (uint32_t t : { 2u, 0u, 2u, (uint32_t)all - 1 }) push_cell(W, D, t / m, t % m);
    CHECK(run(W, labelled(W, D), 0, W.g2_xl, seed, 0).ok == 1, "duplicates and another order");
    { // values as the representative v + r where it fits
        Cells T = C;
        static const uint64_t r[4] = { 0x43E1F593F0000001ULL, 0x2833E84879B97091ULL, 0xB85045B68181585DULL, 0x30644E72E131A029ULL };
        size_t moved = 0;
        for (Fr& v : T.values) {
            unsigned __int128 c = 0;
            Fr s;
            for (int i = 0; i < 4; i++) {
                c += (unsigned __int128)v.d[i] + r[i];
                s.d[i] = (uint64_t)c;
                c >>= 64;
            }
            if (!c) v = s, moved++;
        }
        CHECK(moved > 0 && same(honest, run(W, labelled(W, T), 0, W.g2_xl, seed, 0)), "values as v + r");
    }
    for (size_t t : { (size_t)0, all / 2 + 1, all - 1 }) { // a false value, a wrong proof, a wrong cell index, a wrong label: refused and located
        for (int what = 0; what < 4; what++) {
            Cells T = C;
            if (what == 0) T.values[t * l + (t % l)] = fr_add(T.values[t * l + (t % l)], fr_one());
            else if (what == 1) T.pi[t] = W.rows[1 + t % 3];
            else if (what == 2) T.cell[t] = (uint32_t)((T.cell[t] + 1) % m);
            else T.which[t] = (T.which[t] + 2) % 3;
            if (t / m == 1 && what == 2) continue; // degree < l: every cell has the same remainder and the same proof
            const bbgpu_kzg_check_report R = run(W, labelled(W, T), 0, W.g2_xl, seed, BBGPU_KZG_CHECK_LOCATE);
            CHECK(R.ok == 0 && R.first_failing == (int64_t)t && R.rounds >= 2 && R.rounds <= 9, "l = %zu: tamper %d of cell %zu located (%lld, %u rounds)", l, what, t,
                  (long long)R.first_failing, R.rounds);
            const bbgpu_kzg_check_report Q = run(W, labelled(W, T), 0, W.g2_xl, seed, 0);
            CHECK(Q.ok == 0 && Q.first_failing == -1 && Q.rounds == 1, "cell %zu without the flag", t);
        }
    }
    { // the [x^l] G2 of another power: every cell fails
        const bbgpu_kzg_check_report R = run(W, labelled(W, C), 0, W.g2_other, seed, BBGPU_KZG_CHECK_LOCATE);
        CHECK(R.ok == 0 && R.first_failing == 0, "another g2_xl");
    }
    { // only the cells of the polynomial of degree < l: A and B at infinity
        KzgCellsCall K = O;
        K.commitments = W.commitments[1].w;
        K.values = W.values[n].d;
        K.proofs = W.proofs[m].w;
        const bbgpu_kzg_check_report R = run(W, K, 1, W.g2_xl, seed, 0);
        CHECK(R.ok == 1 && R.a[7] == 1ULL << 63 && R.b[7] == 1ULL << 63, "degree < l: A and B at infinity");
        // the zero polynomial: a commitment at infinity, all-zero cells
        const std::vector<Fr> zeros(n, fr_zero());
        const std::vector<Point> infs(m, INF);
        K.commitments = INF.w;
        K.values = zeros[0].d;
        K.proofs = infs[0].w;
        CHECK(run(W, K, 1, W.g2_xl, seed, 0).ok == 1, "the zero polynomial");
        std::vector<Fr> one = zeros;
        one[m + 1] = fr_one();
        K.values = one[0].d;
        const bbgpu_kzg_check_report Q = run(W, K, 1, W.g2_xl, seed, BBGPU_KZG_CHECK_LOCATE);
        CHECK(Q.ok == 0 && Q.first_failing == 1, "an all-zero cell that is not");
    }
    { // findings
        Cells T = C;
        T.pi[0].w[4] ^= 1;
        T.pi[all - 1].w[0] ^= 1;
        bbgpu_kzg_check_report R = run(W, labelled(W, T), 0, W.g2_xl, seed, BBGPU_KZG_CHECK_LOCATE);
        CHECK(R.ok == 0 && R.rounds == 0 && R.bad_points == 2 && R.first_bad == 0 && R.first_bad_is_proof == 1 && R.a[7] == 1ULL << 63, "two proofs off the curve");
        World V = W;
        V.commitments[2].w[0] ^= 1;
        R = run(V, labelled(V, T), 0, W.g2_xl, seed, 0);
        CHECK(R.ok == 0 && R.bad_points == 3 && R.first_bad == 2 && R.first_bad_is_proof == 0, "a shared commitment before every cell");
    }
    { // the key check
        CHECK(kzg_cells_key_ok(W.rows[0].w, l, W.g2_x, W.g2_xl), "the honest key");
        CHECK(!kzg_cells_key_ok(W.rows[1].w, l, W.g2_x, W.g2_xl), "a head shifted by one row");
        CHECK(!kzg_cells_key_ok(W.rows[0].w, l, W.g2_x, W.g2_other), "the g2_xl of another power");
        uint64_t off[16];
        memcpy(off, W.g2_xl, 128);
        off[8] ^= 1;
        CHECK(!kzg_cells_key_ok(W.rows[0].w, l, W.g2_x, off), "a point off the twist");
    }
    { // the argument verdicts
        bbgpu_kzg_check_report R;
        char why[160];
        auto verdict = [&](KzgCellsCall K, size_t nn, size_t ll, int bt, const uint64_t* g2, int flags) { return kzg_cells_args(&K, nn, ll, bt, g2, flags, &R, why, sizeof why); };
        const KzgCellsCall K = labelled(W, C);
        CHECK(verdict(K, n, l, 0, W.g2_xl, 0) == BBGPU_OK, "a good call");
        CHECK(verdict(K, n, 3, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE && verdict(K, n, 128, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE && verdict(K, l, l, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE &&
                  verdict(K, 12, l, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE && verdict(K, (size_t)1 << 22, l, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE,
              "sizes");
        CHECK(verdict(O, n, l, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE && verdict(O, n, l, 65, W.g2_xl, 0) == BBGPU_ERR_SIZE && verdict(O, n, l, batch, W.g2_xl, 0) == BBGPU_OK, "batch");
        KzgCellsCall B = K;
        B.count = 0;
        CHECK(verdict(B, n, l, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE, "no cells");
        B.count = ((size_t)1 << 20) / l + 1;
        CHECK(verdict(B, n, l, 0, W.g2_xl, 0) == BBGPU_ERR_SIZE, "more than 2^20 values");
        B = K;
        B.S = 2;
        CHECK(verdict(B, n, l, 0, W.g2_xl, 0) == BBGPU_ERR_ARG, "a label out of range");
        B.S = 65;
        CHECK(verdict(B, n, l, 0, W.g2_xl, 0) == BBGPU_ERR_ARG, "65 commitments");
        Cells T = C;
        T.cell[5] = (uint32_t)m;
        CHECK(verdict(labelled(W, T), n, l, 0, W.g2_xl, 0) == BBGPU_ERR_ARG && strstr(why, "cell 5"), "a cell index out of range: %s", why);
        CHECK(verdict(K, n, l, 0, W.g2_xl, 2) == BBGPU_ERR_ARG && verdict(K, n, l, 0, nullptr, 0) == BBGPU_ERR_ARG, "flags, null g2_xl");
        uint64_t bad[16];
        memcpy(bad, W.g2_xl, 128);
        bad[0] ^= 1;
        CHECK(verdict(K, n, l, 0, bad, 0) == BBGPU_ERR_ARG, "g2_xl off the twist");
        std::vector<Point> head(W.rows.begin(), W.rows.begin() + l);
        head[l - 1].w[4] ^= 1;
        B = K;
        B.head = head[0].w;
        CHECK(verdict(B, n, l, 0, W.g2_xl, 0) == BBGPU_ERR_ARG && strstr(why, "off the curve"), "a head row off the curve: %s", why);
        head[l - 1] = INF;
        CHECK(verdict(B, n, l, 0, W.g2_xl, 0) == BBGPU_ERR_ARG && strstr(why, "infinity"), "a head row at infinity: %s", why);
    }
}

int main()
{
    cases(16, 4, 4);
    cases(128, 7, 64);
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
