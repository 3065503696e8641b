// Stand-alone check (own main, no library) of the WIDE quotient-digit forms of barretenberg_amd/csrc/fe.hpp -- the C++ definition the host runs
// and the device's asm forms are compared with -- against big-integer arithmetic.  For Fq and Fr and each of the seven forms (mul, sqr,
// a b + c d, the two in-place forms, the two addhi forms), on operands at the corners of what the form accepts:
//   * the result r satisfies  r 2^261 == a b [+ c d] + q p [+ e 2^261]  EXACTLY (so r == (a b + c d) R^-1 + e modulo p), has exact limbs, lies
//     below the declared bound mul_v(V1, V2) p [+ e], and to_canonical(r) is r mod p;
//   * the 64-bit column accumulator never wraps: the same column walk in 128 bits beside it stays below 2^64 and gives the same limbs,
//     also with ALL NINE limbs of every operand at the form's maximum L U - 1 (the worst case columns_fit() prices);
//   * the quotient is below 2^261 (1 + 2^-26), which is what keeps the value bounds of the masked form.
// Built with -fsanitize=address,undefined by tests/test_fe_wideq_host.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../barretenberg_amd/csrc/fe.hpp"

using namespace bbgpu;
typedef unsigned __int128 u128;

static int fails = 0;
static long checks = 0;
#define CHECK(c, ...) do { checks++; if (!(c)) { if (fails < 40) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } fails++; } } while (0)

// ---- big integers: 26 x 32 bits, unsigned ----
struct Big {
    static const int N = 26;
    uint32_t w[N];
    Big() { memset(w, 0, sizeof w); }
};
static Big from_limbs(const uint32_t* d) // sum d[i] 2^(29 i), limbs of any size
{
    Big r;
    for (int i = 0; i < NL; i++) {
        const int bit = 29 * i, j = bit >> 5, s = bit & 31;
        uint64_t v = (uint64_t)d[i] << s, c = 0;
        for (int k = j; k < Big::N && (v || c); k++) {
            uint64_t t = (uint64_t)r.w[k] + (uint32_t)v + c;
            r.w[k] = (uint32_t)t;
            c = t >> 32;
            v >>= 32;
        }
    }
    return r;
}
static Big add(const Big& a, const Big& b)
{
    Big r;
    uint64_t c = 0;
    for (int i = 0; i < Big::N; i++) { uint64_t t = (uint64_t)a.w[i] + b.w[i] + c; r.w[i] = (uint32_t)t; c = t >> 32; }
    if (c) { printf("Big overflow\n"); exit(2); }
    return r;
}
static Big sub(const Big& a, const Big& b) // a >= b
{
    Big r;
    int64_t c = 0;
    for (int i = 0; i < Big::N; i++) { int64_t t = (int64_t)a.w[i] - b.w[i] + c; r.w[i] = (uint32_t)t; c = t >> 32; }
    if (c) { printf("Big underflow\n"); exit(2); }
    return r;
}
static Big mul(const Big& a, const Big& b)
{
    Big r;
    for (int i = 0; i < Big::N; i++) {
        if (!a.w[i]) continue;
        uint64_t c = 0;
        for (int j = 0; j < Big::N; j++) {
            if (i + j >= Big::N) { if (b.w[j] || c) { printf("Big mul overflow\n"); exit(2); } continue; }
            uint64_t t = (uint64_t)a.w[i] * b.w[j] + r.w[i + j] + c;
            r.w[i + j] = (uint32_t)t;
            c = t >> 32;
        }
    }
    return r;
}
static Big small(uint64_t v) { Big r; r.w[0] = (uint32_t)v; r.w[1] = (uint32_t)(v >> 32); return r; }
static Big shl(const Big& a, int bits)
{
    Big r;
    const int ws = bits >> 5, bs = bits & 31;
    for (int i = Big::N - 1; i >= 0; i--) {
        uint64_t v = 0;
        if (i - ws >= 0) v = (uint64_t)a.w[i - ws] << bs;
        if (bs && i - ws - 1 >= 0) v |= a.w[i - ws - 1] >> (32 - bs);
        r.w[i] = (uint32_t)v;
    }
    return r;
}
static int cmp(const Big& a, const Big& b)
{
    for (int i = Big::N - 1; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static void to_exact_limbs(const Big& a, uint32_t (&d)[NL]) // a < 2^261
{
    for (int i = 0; i < NL; i++) {
        const int bit = 29 * i, j = bit >> 5, s = bit & 31;
        uint64_t v = a.w[j] >> s;
        if (j + 1 < Big::N) v |= (uint64_t)a.w[j + 1] << (32 - s);
        d[i] = (uint32_t)v & M29;
    }
}

// ---- the reduction once more, in 128 bits, digits from a p' computed here ----
template <class F> static uint32_t pinv32()
{
    const uint32_t p0 = F::P[0] | (F::P[1] << 29);
    uint32_t x = p0; // p0 x == 1 mod 2^3; each step doubles the bits
    for (int i = 0; i < 5; i++) x *= 2u - p0 * x;
    return 0u - x;
}
struct Ref {
    uint32_t out[NL], m[NL];
    bool fits;      // every column below 2^64
    u128 worst;
};
template <class F> static Ref ref_redc(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, const uint32_t* e)
{
    Ref r;
    r.fits = true;
    r.worst = 0;
    const uint32_t pi = pinv32<F>();
    u128 acc = 0;
    for (int k = 0; k < 2 * NL - 1; k++) {
        for (int i = 0; i < NL; i++) {
            if (k - i < 0 || k - i >= NL) continue;
            acc += (u128)a[i] * b[k - i];
            if (c) acc += (u128)c[i] * d[k - i];
            if (i < k || k >= NL) acc += (u128)r.m[i] * F::P[k - i];
        }
        if (k < NL) {
            const uint32_t q = (uint32_t)acc * pi;
            r.m[k] = k < NL - 1 ? q : (q & M29);
            acc += (u128)r.m[k] * F::P[0];
            CHECK(((uint32_t)acc & M29) == 0, "column %d does not vanish", k);
        } else {
            if (e) acc += e[k - NL];
            r.out[k - NL] = (uint32_t)acc & M29;
        }
        if (acc > r.worst) r.worst = acc;
        if (acc >> 64) r.fits = false;
        acc >>= 29;
    }
    r.out[NL - 1] = (uint32_t)acc + (e ? e[NL - 1] : 0u);
    return r;
}

template <class F> static Big modulus() { return from_limbs(F::P); }

// ---- the forms ----
enum Form { MUL, SQR, MUL2, MUL_IP, MUL2_IP, MUL_ADDHI_IP, SQR_ADDHI, NFORMS };
static const char* form_name[NFORMS] = { "mul", "sqr", "mul2", "mul_ip", "mul2_ip", "mul_addhi_ip", "sqr_addhi" };
static bool form_two(Form f) { return f == MUL2 || f == MUL2_IP; }
static bool form_sqr(Form f) { return f == SQR || f == SQR_ADDHI; }
static bool form_addhi(Form f) { return f == MUL_ADDHI_IP || f == SQR_ADDHI; }

template <class F> static void run_form(Form f, const uint32_t (&a)[NL], const uint32_t (&b)[NL], const uint32_t (&c)[NL], const uint32_t (&d)[NL], const uint32_t (&e)[NL], uint32_t (&out)[NL])
{
    uint32_t t[NL];
    switch (f) {
    case MUL: mul_raw<F, true>(a, b, out); break;
    case SQR: sqr_raw<F, true>(a, out); break;
    case MUL2: mul2_raw<F, true>(a, b, c, d, out); break;
    case MUL_IP: memcpy(t, a, sizeof t); mul_raw_inplace<F, true>(t, b); memcpy(out, t, sizeof t); break;
    case MUL2_IP: memcpy(t, c, sizeof t); mul2_raw_inplace<F, true>(a, b, t, d); memcpy(out, t, sizeof t); break;
    case MUL_ADDHI_IP: memcpy(t, a, sizeof t); mul_addhi_raw_inplace<F, true>(t, b, e); memcpy(out, t, sizeof t); break;
    case SQR_ADDHI: sqr_addhi_raw<F, true>(a, e, out); break;
    default: break;
    }
}

// an operand: limbs, the limb class L they are within, and (where it is a valid field value) the smallest V with value < V p
struct Operand {
    uint32_t d[NL];
    int L, V; // V = 0: not below 2^261 -- a column-only operand
};
static const uint32_t U = (1u << 29) + 8;

// the same value with limbs pushed to class L: (L - 1) 2^29 moved down from limb i + 1 into limb i wherever limb i + 1 can lend it
static void lift(uint32_t (&d)[NL], int L)
{
    for (int i = 0; i < NL - 1; i++) {
        const uint32_t k = (uint32_t)(L - 1);
        if (d[i + 1] >= k && (uint64_t)d[i] + ((uint64_t)k << 29) < (uint64_t)L * U) {
            d[i + 1] -= k;
            d[i] += k << 29;
        }
    }
}
template <class F> static Operand value_operand(const Big& v, int L)
{
    Operand o;
    to_exact_limbs(v, o.d);
    lift(o.d, L);
    o.L = L;
    const Big p = modulus<F>();
    int V = 1;
    Big vp = p;
    while (cmp(v, vp) >= 0) { vp = add(vp, p); V++; }
    o.V = V;
    for (int i = 0; i < NL; i++) CHECK(o.d[i] < (uint64_t)L * U, "lift left limb %d outside its class", i);
    CHECK(cmp(from_limbs(o.d), v) == 0, "lift changed the value");
    return o;
}
static Operand max_limbs(int L)
{
    Operand o;
    for (int i = 0; i < NL; i++) o.d[i] = (uint32_t)((uint64_t)L * U - 1);
    o.L = L;
    o.V = 0;
    return o;
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rng()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <class F> static std::vector<Operand> operands(int L)
{
    std::vector<Operand> v;
    const Big p = modulus<F>();
    v.push_back(value_operand<F>(Big(), L));                 // 0
    v.push_back(value_operand<F>(sub(p, small(1)), L));      // p - 1
    Big kp;
    for (int k = 1; k <= MAXV; k++) {                        // every multiple k p the value bound admits, and the value just below the next one
        kp = add(kp, p);
        if (k < MAXV) v.push_back(value_operand<F>(kp, L));
        if (k <= 3 || k == 12 || k == 13 || k == 22 || k == MAXV) v.push_back(value_operand<F>(sub(kp, small(1)), L));
    }
    for (int i = 0; i < 6; i++) {                            // a few seeded values below 6 p (what unpack() delivers) and below 168 p
        Big r;
        for (int j = 0; j < 8; j++) r.w[j] = (uint32_t)rng();
        Operand o = value_operand<F>(r, L);
        if (o.V <= MAXV) v.push_back(o);
    }
    v.push_back(max_limbs(L));                               // all nine limbs at L U - 1: the column bound's own worst case (no field value)
    return v;
}
// addends of the addhi forms: limbs of any size below 2^32
template <class F> static std::vector<Operand> addends()
{
    std::vector<Operand> v;
    const Big p = modulus<F>();
    v.push_back(value_operand<F>(Big(), 1));
    v.push_back(value_operand<F>(mul(p, small(13)), 1));     // K p - x as neg() of a stored coordinate delivers it, tight ...
    v.push_back(value_operand<F>(mul(p, small(13)), 3));     // ... and with the limbs neg() really leaves (L = 3)
    v.push_back(value_operand<F>(sub(mul(p, small(28)), small(1)), 5)); // neg(PPP + 2 Q) of the mixed addition
    v.push_back(value_operand<F>(sub(mul(p, small(28)), small(1)), 7));
    Operand o;                                               // every limb 2^32 - 1: column-only
    for (int i = 0; i < NL; i++) o.d[i] = 0xffffffffu;
    o.L = 8;
    o.V = 0;
    v.push_back(o);
    return v;
}

template <class F> static void check_one(Form f, const Operand& A, const Operand& B, const Operand* C, const Operand* D, const Operand* E, const char* fname)
{
    static const uint32_t zero[NL] = { 0 };
    uint32_t out[NL];
    const uint32_t(&c)[NL] = C ? C->d : zero;
    const uint32_t(&d)[NL] = D ? D->d : zero;
    const uint32_t(&e)[NL] = E ? E->d : zero;
    run_form<F>(f, A.d, B.d, c, d, e, out);
    const Ref r = ref_redc<F>(A.d, B.d, C ? C->d : nullptr, D ? D->d : nullptr, E ? E->d : nullptr);
    CHECK(r.fits, "%s %s: a column needs more than 64 bits (L %d %d)", fname, form_name[f], A.L, B.L);
    CHECK(memcmp(out, r.out, sizeof out) == 0, "%s %s: 64-bit walk differs from the 128-bit walk (L %d %d)", fname, form_name[f], A.L, B.L);
    // exact relation, with the digits of the 128-bit walk:  out 2^261 == a b + c d + q p + e 2^261
    const Big p = modulus<F>();
    const Big q = from_limbs(r.m);
    Big rhs = add(mul(from_limbs(A.d), from_limbs(B.d)), mul(q, p));
    if (C) rhs = add(rhs, mul(from_limbs(C->d), from_limbs(D->d)));
    if (E) rhs = add(rhs, shl(from_limbs(E->d), 261));
    // (the top limb is 32 bits of a possibly larger number only for column-only operands: compare the relation only for field values)
    const bool values = A.V && B.V && (!C || (C->V && D->V)) && (!E || E->V);
    CHECK(cmp(q, add(shl(small(1), 261), shl(small(1), 235))) < 0, "%s %s: quotient not below 2^261 (1 + 2^-26)", fname, form_name[f]);
    if (!values) return;
    int V = form_two(f) ? mul2_v(A.V, B.V, C->V, D->V) : mul_v(A.V, B.V);
    if (E) V += E->V;
    if (V > MAXV) return; // the typed layer refuses this pair
    const Big got = from_limbs(out);
    CHECK(cmp(shl(got, 261), rhs) == 0, "%s %s: r 2^261 != a b + c d + q p + e 2^261 (V %d %d)", fname, form_name[f], A.V, B.V);
    for (int i = 0; i < NL; i++) CHECK(out[i] < (1u << 29), "%s %s: limb %d not exact", fname, form_name[f], i);
    CHECK(cmp(got, mul(p, small((uint64_t)V))) < 0, "%s %s: result not below the declared %d p (V %d %d)", fname, form_name[f], V, A.V, B.V);
    // canonicalisation: r - to_canonical(r) is a multiple of p below V p, to_canonical(r) < p
    Fe<F, 1, MAXV> fe;
    for (int i = 0; i < NL; i++) fe.d[i] = out[i];
    uint32_t w[8];
    to_canonical(fe, w);
    Big canon;
    for (int i = 0; i < 8; i++) canon.w[i] = w[i];
    CHECK(cmp(canon, p) < 0, "%s %s: to_canonical not below p", fname, form_name[f]);
    Big diff = sub(got, canon);
    int steps = 0;
    while (cmp(diff, p) >= 0 && steps <= MAXV) { diff = sub(diff, p); steps++; }
    CHECK(cmp(diff, Big()) == 0, "%s %s: to_canonical(r) != r mod p", fname, form_name[f]);
}

template <class F> static void test_field(const char* fname)
{
    // the limb classes the wide forms accept, from the same constexpr the typed layer selects by
    static_assert(wide_columns_fit<F>(4, true), "ll = 4 fits");
    static_assert(!wide_columns_fit<F>(5, false), "ll = 5 does not: the masked digit keeps those sites");
    CHECK(pinv32<F>() == F::PINV32, "%s: PINV32", fname);
    CHECK((F::PINV32 & M29) == F::PINV, "%s: PINV32 extends PINV", fname);
    std::vector<Operand> ops[5];
    for (int L = 1; L <= 4; L++) ops[L] = operands<F>(L);
    const std::vector<Operand> adds = addends<F>();
    const int pairs[][2] = { { 1, 1 }, { 1, 2 }, { 2, 1 }, { 1, 3 }, { 3, 1 }, { 2, 2 }, { 1, 4 }, { 4, 1 } };
    const long before = checks;
    for (int fi = 0; fi < NFORMS; fi++) {
        const Form f = (Form)fi;
        if (form_sqr(f)) {
            for (int L = 1; L <= 2; L++)
                for (const Operand& A : ops[L]) {
                    if (form_addhi(f)) { for (const Operand& E : adds) check_one<F>(f, A, A, nullptr, nullptr, &E, fname); }
                    else check_one<F>(f, A, A, nullptr, nullptr, nullptr, fname);
                }
        } else if (form_two(f)) {
            // L1 L2 + L3 L4 <= 4
            const int quads[][4] = { { 1, 1, 1, 1 }, { 1, 2, 1, 2 }, { 2, 1, 1, 2 }, { 1, 3, 1, 1 }, { 1, 1, 3, 1 }, { 1, 2, 1, 1 }, { 1, 1, 2, 1 } };
            for (const auto& Q : quads) {
                const std::vector<Operand>&a = ops[Q[0]], &b = ops[Q[1]], &c = ops[Q[2]], &d = ops[Q[3]];
                // all four vectors have the same length and order: walk them at co-prime strides so that every operand meets many others
                const size_t n = a.size();
                for (size_t i = 0; i < n; i++)
                    for (size_t j = 0; j < 5; j++)
                        check_one<F>(f, a[i], b[(i * 7 + j * 31) % n], &c[(i * 3 + j * 17 + 1) % n], &d[(i * 5 + j * 11 + 2) % n], nullptr, fname);
                check_one<F>(f, a[n - 1], b[n - 1], &c[n - 1], &d[n - 1], nullptr, fname); // all four at their limb maxima
            }
        } else {
            for (const auto& P : pairs) {
                const std::vector<Operand>&a = ops[P[0]], &b = ops[P[1]];
                const size_t n = a.size();
                for (size_t i = 0; i < n; i++) {
                    // each operand against: its own position, 0, p - 1, p, 167 p, 168 p - 1 (seven entries from the end: six seeded values and the limb
                    // maxima follow them), the limb maxima, and three strided others
                    const size_t others[] = { i, 0, 1, 2, n - 9, n - 8, n - 1, (i * 7 + 3) % n, (i * 13 + 5) % n, (i * 29 + 11) % n };
                    for (size_t j : others) {
                        if (form_addhi(f)) check_one<F>(f, a[i], b[j], nullptr, nullptr, &adds[(i + j) % adds.size()], fname);
                        else check_one<F>(f, a[i], b[j], nullptr, nullptr, nullptr, fname);
                    }
                }
                if (form_addhi(f)) for (const Operand& E : adds) check_one<F>(f, a[n - 1], b[n - 1], nullptr, nullptr, &E, fname);
            }
        }
    }
    printf("%s: %ld checks, fails so far %d\n", fname, checks - before, fails);
}

// the typed layer picks the wide form exactly where the field admits it and the columns fit, and the two digit forms agree modulo p
template <class F> static void test_selection(const char* fname)
{
    // wide only in a field that admits it (F::WIDE_DIGITS: Fq) and only where the columns fit
    static_assert(Digits<F, 1>::wide == F::WIDE_DIGITS && Digits<F, 4>::wide == F::WIDE_DIGITS && Digits<F, 4, true>::wide == F::WIDE_DIGITS, "");
    static_assert(!Digits<F, 5>::wide && !Digits<F, 6>::wide && !Digits<F, 6, true>::wide, "");
    for (int it = 0; it < 200; it++) {
        uint32_t wa[8], wb[8];
        for (int i = 0; i < 8; i++) { wa[i] = (uint32_t)rng(); wb[i] = (uint32_t)rng(); }
        const auto A = unpack<F>(wa), B = unpack<F>(wb);
        uint32_t w1[NL], w2[NL];
        mul_raw<F, true>(A.d, B.d, w1);
        mul_raw<F, false>(A.d, B.d, w2);
        Fe<F, 1, 3> x, y;
        for (int i = 0; i < NL; i++) { x.d[i] = w1[i]; y.d[i] = w2[i]; }
        uint32_t c1[8], c2[8];
        to_canonical(x, c1);
        to_canonical(y, c2);
        CHECK(memcmp(c1, c2, sizeof c1) == 0, "%s: wide and masked products differ modulo p", fname);
        const auto m = mul(A, B); // L = 1: the wide form in Fq, the masked form in Fr
        CHECK(memcmp(m.d, F::WIDE_DIGITS ? w1 : w2, sizeof w1) == 0, "%s: mul() did not take the form the field admits", fname);
        const auto m6 = mul(add(A, A), add(add(B, B), B)); // L1 L2 = 6: masked
        uint32_t w6[NL];
        mul_raw<F, false>(add(A, A).d, add(add(B, B), B).d, w6);
        CHECK(memcmp(m6.d, w6, sizeof w6) == 0, "%s: mul() at L1 L2 = 6 did not keep the masked form", fname);
    }
}

int main()
{
    test_field<FqP>("fq");
    test_field<FrP>("fr");
    test_selection<FqP>("fq");
    test_selection<FrP>("fr");
    printf(fails ? "FAILED %d of %ld\n" : "ALL OK %d of %ld\n", fails, checks);
    return fails ? 1 : 0;
}
