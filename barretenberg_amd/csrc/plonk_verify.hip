// plonk_verify.hip -- the two device parts of a verify call (include/bbgpu.h: bbgpu_plonk_verify_batch, bbgpu_plonk_verify_multi; one driver in capi.hip)
// that are not an MSM: the per-proof work of waffle::Verifier::verify_proof (verifier.cpp:55-355) and the sums over the batch of the scalars on the shared
// points.  Each is one text in two instantiations: proofs of one circuit (its record a kernel argument), or of several.  The definition both follow is
// host_plonk_verify.hpp's verify_terms (the host twin; the comments there name the reference's lines); the sums A and B are the existing device MSM
// over the rows and scalars written here (capi.hip), the pairing is host code (host_pairing.hpp).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bbgpu_internal.h"
#include "fr_sum_device.hpp"
#include "g1.hpp"
#include "keccak_device.hpp"

namespace bbgpu {

namespace {

// ---- k_verify_terms: ONE PROOF PER THREAD, one wave per workgroup ------------------------------------------------------------------------------------
// A proof's work is one dependent chain -- six transcripts, each hashed after the challenge before it entered the arithmetic -- of about 23 Keccak
// permutations, 700 field products (256 of them the one inversion) and nine curve tests, and proofs are independent: a thread per proof needs no
// exchange between lanes, and a batch of thousands fills the chip with waves.  (A wave per proof would have to spread a 25-lane Keccak state and a
// serial chain of products over 64 lanes.)  The transcript, up to 26 elements = 104 lanes, lives in LDS, lane-major so that the 64 threads of a wave
// read consecutive 8-byte words: the Keccak state and every field element stay in registers under compile-time indices, only the absorb reads the
// message by address.  Field arithmetic is fe.hpp's lazy type in Montgomery-261 form; what is hashed leaves it through one product (by 2^5 from the
// memory form, by 1 from ours), what the MSM reads is multiplied by rho_j read as an integer: s 2^261 rho_j 2^-261 = s rho_j, the memory form of
// s (rho_j 2^-256) -- canonical, exactly what the host twin's fr_mul(s, rho_j) gives.
constexpr int VT = 64;          // threads per workgroup
constexpr int MSG_LANES = 104;  // 26 elements of four 64-bit words
using F2 = Fe<FrP, 1, 2>;       // a product

template <class F, int L1, int V1, int L2, int V2> __device__ __forceinline__ Fe<F, 1, V1 + V2> wadd(const Fe<F, L1, V1>& a, const Fe<F, L2, V2>& b)
{
    return weak(add(a, b));
}
template <class F, int L1, int V1, int L2, int V2> __device__ __forceinline__ Fe<F, 1, V1 + V2 + 1> wsub(const Fe<F, L1, V1>& a, const Fe<F, L2, V2>& b)
{
    return weak(sub(a, b));
}
template <class F> __device__ __forceinline__ FeT<F> fe_small(uint32_t v)
{
    FeT<F> r = fe_zero<F>();
    r.d[0] = v;
    return r;
}
__device__ __forceinline__ F2 sel(bool c, const F2& a, const F2& b)
{
    F2 r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.d[i] = c ? a.d[i] : b.d[i];
    return r;
}
__device__ __forceinline__ void ld8(const uint64_t* p, uint32_t (&w)[8])
{
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 a = q[0], b = q[1];
    w[0] = (uint32_t)a.x; w[1] = (uint32_t)(a.x >> 32); w[2] = (uint32_t)a.y; w[3] = (uint32_t)(a.y >> 32);
    w[4] = (uint32_t)b.x; w[5] = (uint32_t)(b.x >> 32); w[6] = (uint32_t)b.y; w[7] = (uint32_t)(b.y >> 32);
}
__device__ __forceinline__ void st8(uint64_t* p, const uint32_t (&w)[8])
{
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    q[0] = make_ulonglong2(w[0] | ((uint64_t)w[1] << 32), w[2] | ((uint64_t)w[3] << 32));
    q[1] = make_ulonglong2(w[4] | ((uint64_t)w[5] << 32), w[6] | ((uint64_t)w[7] << 32));
}
__device__ __forceinline__ void st_row(uint32_t* row, const uint32_t (&o)[16])
{
    uint4* q = reinterpret_cast<uint4*>(row);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}
// element `e` of the transcript: keccak.c:112-134 writes every 64-bit limb most significant byte first, the sponge reads lanes little-endian
__device__ __forceinline__ void put_element(uint64_t* msg, int e, const uint32_t (&w)[8])
{
#pragma unroll
    for (int k = 0; k < 4; k++) msg[(4 * e + k) * VT] = __builtin_bswap64(w[2 * k] | ((uint64_t)w[2 * k + 1] << 32));
}
// Keccak-256 of the first LANES lanes of the transcript: full blocks of the rate (17 lanes), then the rest with the padding 0x01 .. 0x80
template <int LANES> __device__ __forceinline__ void hash_lanes(const uint64_t* msg, uint64_t (&out)[4])
{
    constexpr int FULL = LANES / 17, REM = LANES % 17;
    uint64_t A[25];
#pragma unroll
    for (int k = 0; k < 25; k++) A[k] = 0;
#pragma unroll
    for (int b = 0; b < FULL; b++) {
#pragma unroll
        for (int i = 0; i < 17; i++) A[i] ^= msg[(17 * b + i) * VT];
        keccak_f1600_device(A);
    }
#pragma unroll
    for (int i = 0; i < REM; i++) A[i] ^= msg[(17 * FULL + i) * VT];
    A[REM] ^= 0x01;
    A[16] ^= 0x8000000000000000ULL;
    keccak_f1600_device(A);
    out[0] = A[0]; out[1] = A[1]; out[2] = A[2]; out[3] = A[3];
}
// challenge.hpp:61-70: the digest read as four words, into Montgomery form (ours: times 2^522 through one product)
template <int LANES> __device__ __forceinline__ F2 challenge(const uint64_t* msg)
{
    uint64_t h[4];
    hash_lanes<LANES>(msg, h);
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 4; k++) { w[2 * k] = (uint32_t)h[k]; w[2 * k + 1] = (uint32_t)(h[k] >> 32); }
    return mul(unpack<FrP>(w), fe_from<FrP>(FrP::RSQ));
}
// a value of ours into the transcript: out of Montgomery form, canonical
template <int L, int V> __device__ __forceinline__ void put_fr(uint64_t* msg, int e, const Fe<FrP, L, V>& v)
{
    uint32_t w[8];
    to_canonical(mul(v, fe_small<FrP>(1)), w);
    put_element(msg, e, w);
}
// dst = v rho, canonical (or zero)
template <int L, int V> __device__ __forceinline__ void put_scalar(uint64_t* dst, const Fe<FrP, L, V>& v, const Fe<FrP, 1, 6>& rho, bool zero)
{
    uint32_t w[8];
    to_canonical(mul(v, rho), w);
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = zero ? 0u : w[k];
    st8(dst, w);
}

// what both instantiations take, then the call's circuits: the one record by value, or the table and a label per proof
struct VerifyArgs {
    const uint64_t* proofs; // count x 120 words
    uint32_t* rows_own;     // count x 9 rows of 64 bytes (Montgomery-261, canonical: what the MSM kernels read), the proof's order
    uint32_t* rows_other;   // count x 2 rows: PI_Z_OMEGA, PI_Z
    uint64_t* scal_own;     // count x 9 x 4 words
    uint64_t* scal_other;   // count x 2 x 4 words
    uint64_t* shared;       // [shared point][proof] x 4 words
    uint32_t* status;       // count
    uint32_t count;
    Seed seed;
    VerifyArgs(const VerifyDeviceBuffers& B, size_t n, const uint64_t sd[4])
        : proofs(B.proofs), rows_own(B.rows_own), rows_other(B.rows_other), scal_own(B.scal_own), scal_other(B.scal_other), shared(B.shared), status(B.status),
          count((uint32_t)n)
    {
        for (int k = 0; k < 4; k++) seed.d[k] = sd[k];
    }
};
struct VerifyUniformArgs : VerifyArgs {
    VerifyRecord rec; // base unused
};
// proof j is of circuit[j], whose constants a thread reads from records[circuit[j]] (bbgpu_internal.h); shared is [slot < max over the circuits of
// num_vk + 1][proof], a proof fills the slots of its own circuit
struct VerifyMixedArgs : VerifyArgs {
    const VerifyRecord* records; // one per circuit of the call
    const uint32_t* circuit;     // count
};

// MIXED false: n, the widget set and the key's size are the launch's (kernel arguments: every branch on them is uniform).  MIXED true: they are the
// thread's own, read from its circuit's record where they are needed, so that the z^n loop and the widget branches diverge inside a wave that holds
// proofs of several circuits; the arithmetic is the same text.
template <bool MIXED> __global__ void __launch_bounds__(VT) k_verify_terms(typename std::conditional<MIXED, VerifyMixedArgs, VerifyUniformArgs>::type P)
{
    __shared__ uint64_t s_msg[MSG_LANES * VT];
    const uint32_t j = blockIdx.x * VT + threadIdx.x;
    if (j >= P.count) return;
    uint64_t* msg = s_msg + threadIdx.x;
    const uint64_t* pw = P.proofs + (size_t)j * BBGPU_PLONK_PROOF_WORDS;
    uint32_t gen[16];
    store_affine_m261(gen, fe_from<Fq>(Fq::GEN_X), fe_from<Fq>(Fq::GEN_Y));

    // ---- the nine points: flag, curve test, transcript, row ---------------------------------------------------------------------------------------
    // transcript element of point i: W_L, W_R, W_O at 0, 2, 4; Z_1 at 6; T_LO, T_MID, T_HI at 8, 10, 12; PI_Z, PI_Z_OMEGA at 22, 24.  Z_1's slot first
    // carries gamma (the transcript of beta), so Z_1 enters below, after beta.
    uint32_t status = 0, inf_mask = 0;
    uint32_t z1_plain[16];
    {
        const FeT<Fq> one = fe_one<Fq>();
        const auto three = add(add(one, one), one);
#pragma unroll 1
        for (int i = 0; i < 9; i++) {
            uint32_t w[16], wx[8], wy[8];
            ld8(pw + 8 * i, wx);
            ld8(pw + 8 * i + 4, wy);
#pragma unroll
            for (int k = 0; k < 8; k++) { w[k] = wx[k]; w[8 + k] = wy[k]; }
            const bool inf = (wy[7] >> 31) != 0;
            const bool must_be_finite = i == 3 || i == 4 || i == 7;
            AffineV<2> a;
            load_affine_m256(a, w);
            const auto d = mul_sub(a.y, a.y, sqr(a.x), a.x); // (y^2 - x^3) R
            const bool on = is_zero_mulout(mul(sub(d, three), one));
            if (inf ? must_be_finite : !on) status |= BBGPU_PLONK_VERIFY_BAD_POINT;
            if (inf) inf_mask |= 1u << i;
            // what the reference hashes: both coordinates out of Montgomery form, the flag bit part of y's integer
            uint32_t px[8], py[8];
            to_canonical(mul(unpack<Fq>(wx), fe_from<Fq>(Fq::M256_TO_PLAIN)), px);
            to_canonical(mul(unpack<Fq>(wy), fe_from<Fq>(Fq::M256_TO_PLAIN)), py);
            if (i == 3) {
#pragma unroll
                for (int k = 0; k < 8; k++) { z1_plain[k] = px[k]; z1_plain[8 + k] = py[k]; }
            } else {
                const int e = i < 3 ? 2 * i : i < 7 ? 2 * i : i == 7 ? 22 : 24;
                put_element(msg, e, px);
                put_element(msg, e + 1, py);
            }
            uint32_t o[16];
            store_affine_m261(o, a.x, a.y);
#pragma unroll
            for (int k = 0; k < 16; k++) o[k] = inf ? gen[k] : o[k];
            st_row(P.rows_own + ((size_t)j * 9 + i) * 16, o);
            if (i >= 7) st_row(P.rows_other + ((size_t)j * 2 + (i == 8 ? 0 : 1)) * 16, o);
        }
    }
    // ---- the evaluations: the word test of fr::eq, into our form, into the transcript (elements 14 .. 20) ---------------------------------------------
    F2 wl, wr, wo, s1, s2, z1s, lin, wo_sh, qmc;
    {
        auto load = [&](int e, int element) -> F2 {
            uint32_t w[8];
            ld8(pw + 72 + 4 * e, w);
            if (e == 3 || e == 4 || e == 6) {
                uint32_t any = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) any |= w[k];
                if (any == 0) status |= BBGPU_PLONK_VERIFY_ZERO_EVAL;
            }
            const Fe<FrP, 1, 6> u = unpack<FrP>(w);
            if (element >= 0) {
                uint32_t pl[8];
                to_canonical(mul(u, fe_from<FrP>(FrP::M256_TO_PLAIN)), pl);
                put_element(msg, element, pl);
            }
            return m256_to_m261<FrP>(u);
        };
        wl = load(0, 14); wr = load(1, 15); wo = load(2, 16); s1 = load(3, 17); s2 = load(4, 18); z1s = load(5, 19); lin = load(6, 20);
        wo_sh = load(9, -1);
        qmc = load(11, -1);
    }
    P.status[j] = status;
    const VerifyRecord* rec = nullptr;
    if constexpr (MIXED) rec = P.records + P.circuit[j];
    uint32_t S, log2n, widgets;
    if constexpr (MIXED) {
        S = rec->num_vk + 1;
        log2n = rec->log2n;
        widgets = rec->widgets;
    } else {
        S = P.rec.num_vk + 1;
        log2n = P.rec.log2n;
        widgets = P.rec.widgets;
    }
    // omega, omega^-1, 1 / n: which = 0, 1, 2
    auto domain = [&](int which) -> F2 {
        if constexpr (MIXED) {
            const uint4* q = reinterpret_cast<const uint4*>(rec->root) + 3 * which; // 12 words per constant, 16-byte aligned (VerifyRecord)
            const uint4 a = q[0], b = q[1], c = q[2];
            const uint32_t d[NL] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x };
            return fe_from<FrP>(d);
        } else {
            const uint32_t(&w)[12] = which == 0 ? P.rec.root : which == 1 ? P.rec.root_inv : P.rec.n_inv;
            const uint32_t d[NL] = { w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8] };
            return fe_from<FrP>(d);
        }
    };
    if (status) { // zeros on finite stand-in rows: nothing of this proof enters a sum
        const uint32_t zero8[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll 1
        for (int i = 0; i < 9; i++) {
            st_row(P.rows_own + ((size_t)j * 9 + i) * 16, gen);
            st8(P.scal_own + ((size_t)j * 9 + i) * 4, zero8);
        }
#pragma unroll 1
        for (int i = 0; i < 2; i++) {
            st_row(P.rows_other + ((size_t)j * 2 + i) * 16, gen);
            st8(P.scal_other + ((size_t)j * 2 + i) * 4, zero8);
        }
#pragma unroll 1
        for (uint32_t k = 0; k < S; k++) st8(P.shared + ((size_t)k * P.count + j) * 4, zero8);
        return;
    }

    // ---- challenges, field values (host_plonk_verify.hpp verify_terms, line for line) ----------------------------------------------------------------
    const F2 one = fe_one<FrP>();
    const F2 gamma = challenge<24>(msg);
    put_fr(msg, 6, gamma);
    const F2 beta = challenge<28>(msg);
    {
        uint32_t px[8], py[8];
#pragma unroll
        for (int k = 0; k < 8; k++) { px[k] = z1_plain[k]; py[k] = z1_plain[8 + k]; }
        put_element(msg, 6, px);
        put_element(msg, 7, py);
    }
    const F2 alpha = challenge<32>(msg);
    const F2 z = challenge<56>(msg);

    F2 z_n = z;
    for (uint32_t i = 0; i < log2n; i++) z_n = sqr(z_n);
    const F2 root = domain(0);
    const auto num = wsub(z_n, one), d1 = wsub(z, one), d2 = wsub(mul(mul(z, root), root), one);
    const F2 d12 = mul(d1, d2);
    const uint64_t r_minus_2[4] = { FrP::P64[0] - 2, FrP::P64[1], FrP::P64[2], FrP::P64[3] };
    const F2 inv = pow_u256<FrP>(F2(mul(d12, num)), r_minus_2);
    const F2 inv_d1 = mul(inv, mul(d2, num)), inv_d2 = mul(inv, mul(d1, num)), inv_num = mul(inv, d12);
    const F2 num_n = mul(num, domain(2));
    const F2 l_1 = mul(num_n, inv_d1), l_nm1 = mul(num_n, inv_d2);
    const F2 inv_vanishing = mul(wsub(z, domain(1)), inv_num);

    const F2 a2 = sqr(alpha), a3 = mul(a2, alpha), a4 = sqr(a2), a5 = mul(a4, alpha);
    const F2 zb = mul(z, beta);
    const auto wlg = wadd(wl, gamma), wrg = wadd(wr, gamma), wog = wadd(wo, gamma);
    const F2 lt = mul(mul(wadd(mul(zb, fe_from<FrP>(FrP::GEN7)), wog), wadd(mul(zb, fe_from<FrP>(FrP::GEN5)), wrg)), wadd(zb, wlg));
    const F2 l1a3 = mul(l_1, a3);
    const auto lt_z1 = wadd(mul(lt, alpha), l1a3);
    const F2 p12z = mul(mul(wadd(mul(s1, beta), wlg), wadd(mul(s2, beta), wrg)), z1s);
    const F2 p12za = mul(p12z, alpha);
    const F2 lt_sigma3 = mul(weak(neg(p12za)), beta);
    const auto te = wsub(wsub(mul(mul(wsub(z1s, one), l_nm1), a2), l1a3), mul(p12za, wog));
    const F2 t_eval = mul(wadd(te, lin), inv_vanishing);
    put_fr(msg, 21, t_eval);
    const F2 nu = challenge<88>(msg);
    const F2 u = challenge<104>(msg);

    const F2 nu2 = sqr(nu), nu3 = mul(nu2, nu), nu4 = sqr(nu2), nu5 = mul(nu4, nu), nu6 = mul(nu5, nu), nu7 = mul(nu6, nu), nu8 = sqr(nu4), nu9 = mul(nu8, nu);
    const F2 nu7u = mul(nu7, u);
    const bool seq = (widgets & BBGPU_PLONK_WIDGET_SEQUENTIAL) != 0, has_bool = (widgets & BBGPU_PLONK_WIDGET_BOOL) != 0,
               mimc = (widgets & BBGPU_PLONK_WIDGET_MIMC) != 0, wo_shifted = seq || mimc;
    const F2 zero = fe_zero<FrP>();
    // batch_evaluation: a widget's term is computed whatever the widget set (uniform over the launch, or the thread's own) and zeroed when it is absent
    const F2 b_shift = sel(wo_shifted, mul(mul(wo_sh, nu8), u), zero);
    const F2 b_mimc = sel(mimc, mul(qmc, sel(wo_shifted, nu9, nu8)), zero);
    const auto batch = wadd(wadd(wadd(wadd(wadd(wadd(wadd(wadd(wadd(t_eval, mul(nu, lin)), mul(nu2, wl)), mul(nu3, wr)), mul(nu4, wo)), mul(nu5, s1)),
                                      mul(nu6, s2)), mul(nu7u, z1s)), b_shift), b_mimc);

    // ---- the multiplier, the scalars ------------------------------------------------------------------------------------------------------------------
    Fe<FrP, 1, 6> rho;
    {
        uint64_t r[4];
        keccak_rho_device(P.seed, (uint64_t)j, r);
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { w[2 * k] = (uint32_t)r[k]; w[2 * k + 1] = (uint32_t)(r[k] >> 32); }
        rho = unpack<FrP>(w);
    }
    auto inf = [&](int i) { return ((inf_mask >> i) & 1u) != 0; };
    uint64_t* so = P.scal_own + (size_t)j * 9 * 4;
    const bool wo_there = wo_shifted && !inf(2);
    put_scalar(so + 4 * 0, nu2, rho, inf(0));
    put_scalar(so + 4 * 1, nu3, rho, inf(1));
    put_scalar(so + 4 * 2, wadd(nu4, sel(wo_there, mul(nu8, u), zero)), rho, inf(2));
    put_scalar(so + 4 * 3, wadd(mul(lt_z1, nu), nu7u), rho, false);
    put_scalar(so + 4 * 4, one, rho, false);
    put_scalar(so + 4 * 5, z_n, rho, inf(5));
    put_scalar(so + 4 * 6, sqr(z_n), rho, inf(6));
    put_scalar(so + 4 * 7, z, rho, false);
    put_scalar(so + 4 * 8, mul(mul(z, domain(0)), u), rho, inf(8));
    put_scalar(P.scal_other + ((size_t)j * 2 + 0) * 4, u, rho, inf(8));
    put_scalar(P.scal_other + ((size_t)j * 2 + 1) * 4, one, rho, false);
    auto shared_at = [&](uint32_t k) { return P.shared + ((size_t)k * P.count + j) * 4; };
    const F2 a4nu = mul(a4, nu), a5nu = mul(a5, nu);
    put_scalar(shared_at(0), nu5, rho, false);
    put_scalar(shared_at(1), nu6, rho, false);
    put_scalar(shared_at(2), mul(lt_sigma3, nu), rho, false);
    put_scalar(shared_at(3), mul(mul(wl, wr), a4nu), rho, false);
    put_scalar(shared_at(4), mul(wl, a4nu), rho, false);
    put_scalar(shared_at(5), mul(wr, a4nu), rho, false);
    put_scalar(shared_at(6), mul(wo, a4nu), rho, false);
    put_scalar(shared_at(7), a4nu, rho, false);
    uint32_t k = 8;
    if (seq) put_scalar(shared_at(k++), mul(wo_sh, a4nu), rho, false);
    if (has_bool) {
        put_scalar(shared_at(k++), mul(wsub(sqr(wl), wl), a5nu), rho, false);
        put_scalar(shared_at(k++), mul(mul(wsub(sqr(wr), wr), a5nu), alpha), rho, false);
        put_scalar(shared_at(k++), mul(mul(wsub(sqr(wo), wo), a5nu), a2), rho, false);
    }
    if (mimc) {
        put_scalar(shared_at(k++), sel(wo_there, nu9, nu8), rho, false);
        const auto t0 = wadd(wadd(wo, wl), qmc);
        const auto cube = wsub(mul(sqr(t0), t0), wr);
        const F2 out = mul(wsub(mul(sqr(wr), t0), wo_sh), alpha);
        put_scalar(shared_at(k++), mul(wadd(out, cube), a5nu), rho, false);
    }
    put_scalar(shared_at(k), weak(neg(batch)), rho, false); // on the generator
}

// ---- k_verify_fold: out[k] = sum over the proofs j < m of shared[k][j], one workgroup per shared point ----------------------------------------------
// Canonical 256-bit additions modulo r: exact, so the fixed tree below gives the value any other order would.  No floating point, no atomics.
constexpr int FT = 256;
// the 256 partial sums of a workgroup into one, by a fixed tree; thread 0 writes it (zero for a key point at infinity: its row is a stand-in)
__device__ __forceinline__ void fold_finish(uint64_t (&s_acc)[FT][4], const uint64_t (&acc)[4], bool skip, uint64_t* __restrict__ dst)
{
#pragma unroll
    for (int i = 0; i < 4; i++) s_acc[threadIdx.x][i] = acc[i];
    __syncthreads();
    for (uint32_t o = FT / 2; o; o >>= 1) {
        if (threadIdx.x < o) {
            uint64_t a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; i++) { a[i] = s_acc[threadIdx.x][i]; b[i] = s_acc[threadIdx.x + o][i]; }
            fr_add_canonical(a, b);
#pragma unroll
            for (int i = 0; i < 4; i++) s_acc[threadIdx.x][i] = a[i];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    ulonglong2* o2 = reinterpret_cast<ulonglong2*>(dst);
    o2[0] = make_ulonglong2(skip ? 0 : s_acc[0][0], skip ? 0 : s_acc[0][1]);
    o2[1] = make_ulonglong2(skip ? 0 : s_acc[0][2], skip ? 0 : s_acc[0][3]);
}
// MIXED false: workgroup k sums slot k over the proofs j < m into out[k].  MIXED true: workgroup (k, c) sums slot k over the proofs j < m labelled c
// into the scalar of circuit c's k-th shared row; a proof of another circuit costs its 4-byte label, not the 32-byte term.
template <bool MIXED> __global__ void __launch_bounds__(FT) k_verify_fold(const uint64_t* __restrict__ shared, const uint32_t* __restrict__ circuit,
                                                                          const VerifyRecord* __restrict__ records, uint32_t count, uint32_t m,
                                                                          uint32_t skip_mask, uint64_t* __restrict__ out)
{
    __shared__ uint64_t s_acc[FT][4];
    const uint32_t k = blockIdx.x, c = blockIdx.y;
    uint32_t base = 0;
    if constexpr (MIXED) {
        const uint32_t num_vk = records[c].num_vk;
        base = records[c].base;
        skip_mask = records[c].skip_mask;
        if (k > num_vk) return; // the whole workgroup: circuit c has no such slot
    }
    uint64_t acc[4] = { 0, 0, 0, 0 };
    for (uint32_t j = threadIdx.x; j < m; j += FT) {
        if constexpr (MIXED)
            if (circuit[j] != c) continue;
        const ulonglong2* q = reinterpret_cast<const ulonglong2*>(shared + ((size_t)k * count + j) * 4);
        const ulonglong2 lo = q[0], hi = q[1];
        const uint64_t v[4] = { lo.x, lo.y, hi.x, hi.y };
        fr_add_canonical(acc, v);
    }
    fold_finish(s_acc, acc, ((skip_mask >> k) & 1u) != 0, out + 4 * (size_t)(base + k));
}

} // namespace

int plonk_verify_terms(const VerifyCircuits& C, const uint64_t seed[4], size_t count, const VerifyDeviceBuffers& B, hipStream_t st)
{
    const uint32_t grid = (uint32_t)((count + VT - 1) / VT);
    if (C.one) k_verify_terms<false><<<grid, VT, 0, st>>>(VerifyUniformArgs{ { B, count, seed }, *C.one });
    else k_verify_terms<true><<<grid, VT, 0, st>>>(VerifyMixedArgs{ { B, count, seed }, C.d_records, C.d_circuit });
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// the sums over the first m proofs: d_out[k] for the shared points of the one circuit, or d_out[records[c].base + k] for every circuit c and slot k of it
int plonk_verify_fold(const VerifyCircuits& C, const uint64_t* d_shared, size_t count, size_t m, uint64_t* d_out, hipStream_t st)
{
    if (C.one) k_verify_fold<false><<<C.one->num_vk + 1, FT, 0, st>>>(d_shared, nullptr, nullptr, (uint32_t)count, (uint32_t)m, C.one->skip_mask, d_out);
    else
        k_verify_fold<true><<<dim3((uint32_t)C.max_shared, (uint32_t)C.num_circuits), FT, 0, st>>>(d_shared, C.d_circuit, C.d_records, (uint32_t)count, (uint32_t)m, 0,
                                                                                                   d_out);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
