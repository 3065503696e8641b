// host_plonk_verify.hpp -- the batched PLONK verifier on the host (include/bbgpu.h, bbgpu_host_plonk_verify_batch) and everything the GPU entry
// (plonk_verify.hip, capi.hip) shares with it: the handle's key, the verdict on its points, the multipliers, the pairing tail with its bisection.
// The per-proof work restates waffle::Verifier::verify_proof (verifier.cpp:55-355) over challenge.hpp, linearizer.hpp,
// polynomial_arithmetic.cpp:594-626 and the four widgets' append_scalar_multiplication_inputs / compute_batch_evaluation_contribution; where the
// reference ends in two pairings per proof (:357-379) a batch of proofs of the circuits under one x G2 (verify_host_multi; of ONE circuit: verify_host, the
// same with one key) is folded with multipliers rho_j into two sums and one product of two pairings, as bbgpu_srs_check folds its row pairs (host_srs_check.hpp).  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bbgpu.h"
#include "host_fallback.hpp"
#include "host_fr.hpp"
#include "host_pairing.hpp"
#include "host_srs_check.hpp"
#include "keccak.hpp"

namespace bbgpu {
namespace host {

constexpr int VERIFY_OWN = 9;         // a proof's own points, in the proof's order: W_L, W_R, W_O, Z_1, T_LO, T_MID, T_HI, PI_Z, PI_Z_OMEGA
constexpr int VERIFY_MAX_SHARED = 13; // the key's 8 to 12 points, then the generator
enum { VP_W_L = 0, VP_W_R, VP_W_O, VP_Z_1, VP_T_LO, VP_T_MID, VP_T_HI, VP_PI_Z, VP_PI_Z_OMEGA };
// the proof's evaluations, 4 words each from word 72 on (waffle_types.hpp:18-45)
enum { VE_W_L = 0, VE_W_R, VE_W_O, VE_SIGMA_1, VE_SIGMA_2, VE_Z_1_SHIFTED, VE_LINEAR, VE_W_L_SHIFTED, VE_W_R_SHIFTED, VE_W_O_SHIFTED, VE_Q_C, VE_Q_MIMC_COEFFICIENT };

// what bbgpu_plonk_verifier_create keeps: the key as given, which of its points are the point at infinity (a selector that is identically zero
// commits to it, tests/golden/infinity_commitments.json; the reference skips such a point, arithmetic_widget.cpp:197-237), and the domain's constants
struct VerifyKey {
    size_t n = 0;
    int log2n = 0, widgets = 0, num_vk = 0;
    uint64_t vk[BBGPU_PLONK_VK_WORDS] = {};
    bool vk_inf[12] = {};
    uint64_t g2_x[16] = {};
    Fr root, root_inv, n_inv; // omega, omega^-1, 1 / n (evaluation_domain.cpp)
    int num_shared() const { return num_vk + 1; }
};

static inline int verify_num_vk(int widgets)
{
    return 8 + ((widgets & BBGPU_PLONK_WIDGET_SEQUENTIAL) ? 1 : 0) + ((widgets & BBGPU_PLONK_WIDGET_BOOL) ? 3 : 0) + ((widgets & BBGPU_PLONK_WIDGET_MIMC) ? 2 : 0);
}
static inline bool verify_widgets_ok(int w)
{
    return w == 0 || w == BBGPU_PLONK_WIDGET_BOOL || w == BBGPU_PLONK_WIDGET_MIMC || w == BBGPU_PLONK_WIDGET_SEQUENTIAL ||
           w == (BBGPU_PLONK_WIDGET_SEQUENTIAL | BBGPU_PLONK_WIDGET_BOOL);
}
static inline Fr fr_canonical(Fr a) // any 256-bit value: 2^256 < 6 r
{
    for (int i = 0; i < 5; i++) fr_cond_sub_p(a);
    return a;
}

// BBGPU_OK, or the argument error of bbgpu_plonk_verifier_create / bbgpu_host_plonk_verify_batch (*why: a text for bbgpu_last_error)
static inline int verify_key_init(VerifyKey* K, size_t n, int widgets, const uint64_t* vk, const uint64_t* g2_x, const char** why)
{
    if (!vk || !g2_x) { *why = "null verification key or g2_x"; return BBGPU_ERR_ARG; }
    if (!verify_widgets_ok(widgets)) { *why = "unknown widget set (none, bool, MiMC, sequential, sequential + bool)"; return BBGPU_ERR_ARG; }
    int lg = 0;
    while (lg < 28 && ((size_t)1 << lg) < n) lg++;
    if (n < 2 || ((size_t)1 << lg) != n) { *why = "n is not 2^k, 1 <= k <= 28"; return BBGPU_ERR_SIZE; }
    if (!srs_check_g2_ok(g2_x)) { *why = "g2_x is not a point of order r on the twist"; return BBGPU_ERR_ARG; }
    K->n = n;
    K->log2n = lg;
    K->widgets = widgets;
    K->num_vk = verify_num_vk(widgets);
    memset(K->vk, 0, sizeof K->vk);
    memcpy(K->vk, vk, (size_t)K->num_vk * 64);
    memcpy(K->g2_x, g2_x, 128);
    for (int k = 0; k < K->num_vk; k++) {
        K->vk_inf[k] = g1_words_is_inf(vk + 8 * k);
        if (!K->vk_inf[k] && !g1_words_on_curve(vk + 8 * k)) { *why = "a point of the verification key is not on the curve"; return BBGPU_ERR_ARG; }
    }
    K->root = fr_root_of_unity(lg);
    K->root_inv = fr_inv(K->root);
    K->n_inv = fr_inv(fr_from_u64((uint64_t)n));
    return BBGPU_OK;
}

// what one proof contributes: the scalars on its own points, the two of the other side (u on PI_Z_OMEGA, 1 on PI_Z), one per shared point -- all
// already multiplied by rho_j, Montgomery, canonical; zeros when status != 0
struct VerifyTerms {
    uint32_t status;
    Fr own[VERIFY_OWN], other[2], shared[VERIFY_MAX_SHARED];
};

static inline Fr verify_challenge(const uint64_t* buf, size_t elements)
{
    Fr raw;
    hash_field_elements(buf, elements, raw.d);
    return fr_to_mont(raw);
}

static inline void verify_terms(const VerifyKey& K, const uint64_t* pw, const uint64_t rho_words[4], VerifyTerms* T)
{
    memset(T, 0, sizeof *T);
    bool inf[VERIFY_OWN];
    for (int i = 0; i < VERIFY_OWN; i++) {
        const uint64_t* p = pw + 8 * i;
        inf[i] = g1_words_is_inf(p);
        const bool must_be_finite = i == VP_Z_1 || i == VP_T_LO || i == VP_PI_Z;
        if (inf[i] ? must_be_finite : !g1_words_on_curve(p)) T->status |= BBGPU_PLONK_VERIFY_BAD_POINT;
    }
    const uint64_t* ew = pw + 72;
    // fr::eq(x, fr::zero) compares the four words (field.hpp:166-170): the representative r of zero is NOT zero there, and not here
    for (int e : { (int)VE_SIGMA_1, (int)VE_SIGMA_2, (int)VE_LINEAR })
        if ((ew[4 * e] | ew[4 * e + 1] | ew[4 * e + 2] | ew[4 * e + 3]) == 0) T->status |= BBGPU_PLONK_VERIFY_ZERO_EVAL;
    if (T->status) return;

    Fr ev[12];
    for (int e = 0; e < 12; e++) {
        memcpy(ev[e].d, ew + 4 * e, 32);
        ev[e] = fr_canonical(ev[e]);
    }
    // the transcript (challenge.hpp:15-59): every element out of Montgomery form, the flag bit of an infinite point's y included as the reference includes it
    uint64_t buf[26 * 4];
    const Fq fq_one_raw = { { 1, 0, 0, 0 } };
    auto put_point = [&](int element, int point) {
        for (int c = 0; c < 2; c++) {
            Fq v;
            memcpy(v.d, pw + 8 * point + 4 * c, 32);
            v = fq_mul(v, fq_one_raw);
            memcpy(buf + 4 * (element + c), v.d, 32);
        }
    };
    auto put_fr = [&](int element, const Fr& v) {
        const Fr plain = fr_from_mont(v);
        memcpy(buf + 4 * element, plain.d, 32);
    };
    put_point(0, VP_W_L);
    put_point(2, VP_W_R);
    put_point(4, VP_W_O);
    const Fr gamma = verify_challenge(buf, 6);
    put_fr(6, gamma);
    const Fr beta = verify_challenge(buf, 7);
    put_point(6, VP_Z_1);
    const Fr alpha = verify_challenge(buf, 8);
    put_point(8, VP_T_LO);
    put_point(10, VP_T_MID);
    put_point(12, VP_T_HI);
    const Fr z = verify_challenge(buf, 14);

    const Fr one = fr_one();
    const Fr &wl = ev[VE_W_L], &wr = ev[VE_W_R], &wo = ev[VE_W_O], &s1 = ev[VE_SIGMA_1], &s2 = ev[VE_SIGMA_2], &z1s = ev[VE_Z_1_SHIFTED], &lin = ev[VE_LINEAR];
    const Fr &wo_sh = ev[VE_W_O_SHIFTED], &qmc = ev[VE_Q_MIMC_COEFFICIENT];
    // Z_H*(z) = (z^n - 1) / (z - w^-1), L_1(z) = (z^n - 1) / (n (z - 1)), L_{n-1}(z) = (z^n - 1) / (n (z w^2 - 1)); t_eval divides by Z_H*(z): ONE inversion,
    // of (z - 1)(z w^2 - 1)(z^n - 1) (zero gives zero, as fr::invert does; a challenge hits a zero with probability ~2^-225)
    Fr z_n = z;
    for (int i = 0; i < K.log2n; i++) z_n = fr_sqr(z_n);
    const Fr num = fr_sub(z_n, one), d1 = fr_sub(z, one), d2 = fr_sub(fr_mul(fr_mul(z, K.root), K.root), one);
    const Fr d12 = fr_mul(d1, d2);
    const Fr inv = fr_inv_fermat(fr_mul(d12, num));
    const Fr inv_d1 = fr_mul(inv, fr_mul(d2, num)), inv_d2 = fr_mul(inv, fr_mul(d1, num)), inv_num = fr_mul(inv, d12);
    const Fr num_n = fr_mul(num, K.n_inv);
    const Fr l_1 = fr_mul(num_n, inv_d1), l_nm1 = fr_mul(num_n, inv_d2);
    const Fr inv_vanishing = fr_mul(fr_sub(z, K.root_inv), inv_num);

    const Fr a2 = fr_sqr(alpha), a3 = fr_mul(a2, alpha), a4 = fr_sqr(a2), a5 = fr_mul(a4, alpha);
    // linearizer.hpp:29-85
    const Fr zb = fr_mul(z, beta);
    const Fr wlg = fr_add(wl, gamma), wrg = fr_add(wr, gamma), wog = fr_add(wo, gamma);
    Fr lt_z1 = fr_mul(fr_mul(fr_add(fr_mul(zb, fr_from_limbs(FrHostP::GEN7)), wog), fr_add(fr_mul(zb, fr_from_limbs(FrHostP::GEN5)), wrg)), fr_add(zb, wlg));
    lt_z1 = fr_add(fr_mul(lt_z1, alpha), fr_mul(l_1, a3));
    const Fr p1 = fr_add(fr_mul(s1, beta), wlg), p2 = fr_add(fr_mul(s2, beta), wrg);
    const Fr p12z = fr_mul(fr_mul(p1, p2), z1s);
    const Fr lt_sigma3 = fr_mul(fr_neg(fr_mul(p12z, alpha)), beta);
    // verifier.cpp:131-158
    Fr t_eval = fr_mul(fr_mul(p12z, wog), alpha);
    t_eval = fr_sub(fr_sub(fr_mul(fr_mul(fr_sub(z1s, one), l_nm1), a2), fr_mul(l_1, a3)), t_eval);
    t_eval = fr_mul(fr_add(t_eval, lin), inv_vanishing);

    for (int e = 0; e < 7; e++) put_fr(14 + e, ev[e]);
    put_fr(21, t_eval);
    const Fr nu = verify_challenge(buf, 22);
    put_point(22, VP_PI_Z);
    put_point(24, VP_PI_Z_OMEGA);
    const Fr u = verify_challenge(buf, 26);

    Fr nup[10]; // nup[i] = nu^i
    nup[0] = one;
    for (int i = 1; i < 10; i++) nup[i] = fr_mul(nup[i - 1], nu);
    const Fr nu7u = fr_mul(nup[7], u);
    // verifier.cpp:186-252
    Fr batch = t_eval;
    batch = fr_add(batch, fr_mul(nup[1], lin));
    batch = fr_add(batch, fr_mul(nup[2], wl));
    batch = fr_add(batch, fr_mul(nup[3], wr));
    batch = fr_add(batch, fr_mul(nup[4], wo));
    batch = fr_add(batch, fr_mul(nup[5], s1));
    batch = fr_add(batch, fr_mul(nup[6], s2));
    batch = fr_add(batch, fr_mul(nu7u, z1s));
    const bool wo_shifted = (K.widgets & (BBGPU_PLONK_WIDGET_SEQUENTIAL | BBGPU_PLONK_WIDGET_MIMC)) != 0;
    Fr nu_base = nup[8];
    if (wo_shifted) {
        batch = fr_add(batch, fr_mul(fr_mul(wo_sh, nu_base), u));
        nu_base = nup[9];
    }
    if (K.widgets & BBGPU_PLONK_WIDGET_MIMC) batch = fr_add(batch, fr_mul(qmc, nu_base));

    Fr own[VERIFY_OWN], shared[VERIFY_MAX_SHARED];
    own[VP_Z_1] = fr_add(fr_mul(lt_z1, nu), nu7u);
    own[VP_W_L] = nup[2];
    own[VP_W_R] = nup[3];
    own[VP_W_O] = nup[4];
    // verifier.cpp:264-313: the base of the widgets' opening scalars advances only past a W_O that is there
    Fr nu_base_points = nup[8];
    if (wo_shifted && !inf[VP_W_O]) {
        own[VP_W_O] = fr_add(own[VP_W_O], fr_mul(nup[8], u));
        nu_base_points = nup[9];
    }
    own[VP_PI_Z_OMEGA] = fr_mul(fr_mul(z, K.root), u);
    own[VP_PI_Z] = z;
    own[VP_T_LO] = one;
    own[VP_T_MID] = z_n;
    own[VP_T_HI] = fr_sqr(z_n);
    shared[0] = nup[5];
    shared[1] = nup[6];
    shared[2] = fr_mul(lt_sigma3, nu);
    // arithmetic_widget.cpp:186-246 at alpha_base = alpha^4
    const Fr a4nu = fr_mul(a4, nu), a5nu = fr_mul(a5, nu);
    shared[3] = fr_mul(fr_mul(wl, wr), a4nu);
    shared[4] = fr_mul(wl, a4nu);
    shared[5] = fr_mul(wr, a4nu);
    shared[6] = fr_mul(wo, a4nu);
    shared[7] = a4nu;
    int k = 8;
    if (K.widgets & BBGPU_PLONK_WIDGET_SEQUENTIAL) shared[k++] = fr_mul(wo_sh, a4nu); // sequential_widget.cpp:122-149: alpha_base / alpha_step = alpha^4
    if (K.widgets & BBGPU_PLONK_WIDGET_BOOL) { // bool_widget.cpp:188-225 at alpha_base = alpha^5
        shared[k++] = fr_mul(fr_sub(fr_sqr(wl), wl), a5nu);
        shared[k++] = fr_mul(fr_mul(fr_sub(fr_sqr(wr), wr), a5nu), alpha);
        shared[k++] = fr_mul(fr_mul(fr_sub(fr_sqr(wo), wo), a5nu), a2);
    }
    if (K.widgets & BBGPU_PLONK_WIDGET_MIMC) { // mimc_widget.cpp:180-213 at alpha_base = alpha^5
        shared[k++] = nu_base_points;
        const Fr t0 = fr_add(fr_add(wo, wl), qmc);
        const Fr cube = fr_sub(fr_mul(fr_sqr(t0), t0), wr);
        const Fr out = fr_mul(fr_sub(fr_mul(fr_sqr(wr), t0), wo_sh), alpha);
        shared[k++] = fr_mul(fr_add(out, cube), a5nu);
    }
    shared[k++] = fr_neg(batch); // on the generator
    Fr rho;
    memcpy(rho.d, rho_words, 32);
    for (int i = 0; i < VERIFY_OWN; i++) T->own[i] = inf[i] ? fr_zero() : fr_mul(own[i], rho);
    T->other[0] = inf[VP_PI_Z_OMEGA] ? fr_zero() : fr_mul(u, rho);
    T->other[1] = rho;
    for (int i = 0; i < k; i++) T->shared[i] = fr_mul(shared[i], rho);
}

static inline void verify_report_init(bbgpu_plonk_verify_report* R, size_t count, const uint64_t seed[4])
{
    memset(R, 0, sizeof(*R));
    R->count = count;
    R->first_bad_status = UINT64_MAX;
    R->first_bad_proof = UINT64_MAX;
    report_no_sums(seed, R->seed, R->a, R->b);
}

// e(A, G2) e(-B, x G2) == 1 (verifier.cpp:360-379 with reference_string.cpp:27-28: the sum with T_LO meets G2, the negated openings meet x G2)
static inline bool verify_pair(const uint64_t a12[12], const uint64_t b12[12], const uint64_t g2_x[16]) { return pair_is_one(a12, b12, &G2_ONE, g2_x); }

// The tail once every status is known, through prefix_check.  sums(m, a12, b12): A and B over the proofs [0, m).  The sums run over the proofs with status 0
// (the others contribute zeros), the verdict on the batch needs both.  With BBGPU_PLONK_VERIFY_LOCATE the first failing prefix ends in the first bad proof.
template <class Sums> static inline int verify_tail(bbgpu_plonk_verify_report* R, const uint64_t g2_x[16], int flags, Sums sums)
{
    PrefixVerdict v;
    const int rc = prefix_check((size_t)R->count, (flags & BBGPU_PLONK_VERIFY_LOCATE) != 0, sums,
                                [&](const uint64_t* a12, const uint64_t* b12) { return verify_pair(a12, b12, g2_x); }, &v);
    if (!v.rounds) return rc;
    memcpy(R->a, v.a, 64);
    memcpy(R->b, v.b, 64);
    R->pairing_checked = 1;
    R->pairing_ok = v.ok ? 1 : 0;
    if (v.first_failing != SIZE_MAX) R->first_bad_proof = v.first_failing;
    return rc;
}

static inline void verify_count_status(bbgpu_plonk_verify_report* R, const uint32_t* status)
{
    for (size_t j = 0; j < (size_t)R->count; j++)
        if (status[j] && R->bad_status++ == 0) R->first_bad_status = j;
}

// the key's points and the generator as the sums take them: 64 bytes each, an infinite key point replaced by the generator (its scalar is zero)
static inline void verify_shared_points(const VerifyKey& K, uint64_t* out /* num_shared x 8 */)
{
    for (int k = 0; k < K.num_shared(); k++) {
        if (k < K.num_vk && !K.vk_inf[k]) memcpy(out + 8 * k, K.vk + 8 * k, 64);
        else g1_generator_words(out + 8 * k);
    }
}
// a proof's point as a sum takes it: canonical coordinates; the generator where the flag is set (its scalar is zero)
static inline void verify_own_point(const uint64_t* p, uint64_t out[8])
{
    if (g1_words_is_inf(p)) return g1_generator_words(out);
    Fq x, y;
    g1_words_canonical(p, &x, &y);
    memcpy(out, x.d, 32);
    memcpy(out + 4, y.d, 32);
}

// bbgpu_host_plonk_verify_multi behind its argument checks: proof j is of keys[circuit[j]]; every key under g2_x.  The rows of A are all circuits' shared
// rows (circuit c's from base_c = sum of the num_shared() before it), then nine per proof in the caller's order; the scalar on V_{c,k} collects the
// terms of the proofs labelled c.  A null `circuit` labels every proof 0.
static inline int verify_host_multi(const VerifyKey* keys, size_t num, const uint64_t g2_x[16], const uint32_t* circuit, const uint64_t* proofs, size_t count,
                                    const uint64_t seed[4], int flags, uint32_t* status, bbgpu_plonk_verify_report* R)
{
    verify_report_init(R, count, seed);
    auto label = [&](size_t j) -> size_t { return circuit ? circuit[j] : 0; };
    std::vector<size_t> base(num);
    size_t T = 0;
    for (size_t c = 0; c < num; c++) {
        base[c] = T;
        T += (size_t)keys[c].num_shared();
    }
    std::vector<VerifyTerms> terms(count);
    std::vector<uint64_t> pts_a((T + VERIFY_OWN * count) * 8), pts_b(2 * count * 8);
    for (size_t c = 0; c < num; c++) verify_shared_points(keys[c], pts_a.data() + 8 * base[c]);
    const uint64_t* gen = pts_a.data() + 8 * (base[0] + keys[0].num_shared() - 1); // the generator: the last shared row of every circuit
    fallback_parallel(count, 4, [&](size_t lo, size_t hi) {
        for (size_t j = lo; j < hi; j++) {
            uint64_t rho[4];
            srs_check_rho(seed, j, rho);
            const uint64_t* pw = proofs + BBGPU_PLONK_PROOF_WORDS * j;
            verify_terms(keys[label(j)], pw, rho, &terms[j]);
            status[j] = terms[j].status;
            for (int i = 0; i < VERIFY_OWN; i++) verify_own_point(terms[j].status ? gen : pw + 8 * i, &pts_a[(T + VERIFY_OWN * j + i) * 8]);
            for (int i = 0; i < 2; i++) verify_own_point(terms[j].status ? gen : pw + 8 * (i == 0 ? VP_PI_Z_OMEGA : VP_PI_Z), &pts_b[(2 * j + i) * 8]);
        }
    });
    verify_count_status(R, status);
    std::vector<uint64_t> sc_a((T + VERIFY_OWN * count) * 4), sc_b(2 * count * 4);
    for (size_t j = 0; j < count; j++) {
        memcpy(&sc_a[(T + VERIFY_OWN * j) * 4], terms[j].own, VERIFY_OWN * 32);
        memcpy(&sc_b[2 * j * 4], terms[j].other, 64);
    }
    return verify_tail(R, g2_x, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) {
        std::vector<Fr> acc(T, fr_zero());
        for (size_t j = 0; j < m; j++) {
            const VerifyKey& K = keys[label(j)];
            Fr* a = &acc[base[label(j)]];
            for (int k = 0; k < K.num_shared(); k++)
                if (k == K.num_vk || !K.vk_inf[k]) a[k] = fr_add(a[k], terms[j].shared[k]);
        }
        memcpy(sc_a.data(), acc.data(), T * 32);
        g1_to_normalised(msm_pippenger(sc_a.data(), pts_a.data(), T + VERIFY_OWN * m, 8), a12);
        g1_to_normalised(msm_pippenger(sc_b.data(), pts_b.data(), 2 * m, 8), b12);
        return (int)BBGPU_OK;
    });
}

// bbgpu_host_plonk_verify_batch behind its argument checks: one key, every proof of it
static inline int verify_host(const VerifyKey& K, const uint64_t* proofs, size_t count, const uint64_t seed[4], int flags, uint32_t* status,
                              bbgpu_plonk_verify_report* R)
{
    return verify_host_multi(&K, 1, K.g2_x, nullptr, proofs, count, seed, flags, status, R);
}

} // namespace host
} // namespace bbgpu
