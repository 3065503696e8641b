// kzg_check.hip -- the two device parts of a check of KZG openings (include/bbgpu.h: bbgpu_kzg_check_openings, bbgpu_kzg_check_open_all; one driver in
// capi.hip) that are not an MSM: the per-claim rows, scalars and terms, and the sums over the claims of the scalars on G and on the shared commitments.
// The definition both follow is host_kzg_check_batch.hpp's kzg_check_host (the host twin); the sums A and B are the existing device MSM over the rows
// and scalars written here, the pairing is host code (host_pairing.hpp).  The reference has no batched check of openings.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "fr_mem_device.hpp"
#include "fr_sum_device.hpp"
#include "g1.hpp"
#include "keccak_device.hpp"

namespace bbgpu {

namespace {

constexpr int CT = 256; // threads per workgroup, every kernel here
using F2 = Fe<FrP, 1, 2>; // a product

// ---- k_kzg_claims: ONE CLAIM PER THREAD, strided ---------------------------------------------------------------------------------------------------------
// A claim is independent of every other: one Keccak permutation (rho_t), one or two curve tests (k_srs_on_curve's: y y + (K p - x^2) x in one shared
// reduction, minus 3 R, one more product, is_zero_mulout), the rows in the form the MSM kernels read, and three products by rho_t READ AS AN INTEGER:
// v 2^261 rho 2^-261 = v rho, the memory form of v (rho 2^-256) -- canonical, exactly what the host twin's fr_mul(v, rho) gives.  A point at infinity
// becomes the generator under scalar zero, as in k_verify_terms.  Findings meet on chip -- shuffles inside a wave, an LDS slot per wave -- and ONE thread
// per workgroup issues the count atomicAdd and the first-key atomicMin, only if the workgroup found anything: an honest call issues no atomic, and sums
// and minima do not depend on arrival order.  The key of a finding is 2 t + (1 for the proof): C_t before pi_t before claim t + 1.
struct KzgClaimsArgs {
    const uint64_t* proofs;      // count x 8 words, the caller's
    const uint64_t* commitments; // PER_CLAIM: count x 8 words
    const uint64_t* z;           // count x 4 words (not OPEN_ALL)
    const uint64_t* y;           // count x 4 words
    uint32_t* rows;              // the claims' rows: PER_CLAIM (C_t, pi_t), else pi_t; 64 bytes each, Montgomery-261, canonical
    uint64_t *scal_a, *scal_b;   // the scalars of A and of B on those rows
    uint64_t *term_y, *term_rho; // rho_t y_t; rho_t (shared layouts: what the fold adds up per commitment)
    KzgFindings* find;
    uint64_t count;
    uint32_t log2n;              // OPEN_ALL: z_t = omega^(t mod 2^log2n)
    Limbs9 omega, step;          // omega and omega^(threads of the grid), Montgomery-261
    Seed seed;
};

// reads a point in the reference's format, tests it, writes its row; returns the infinity flag
__device__ __forceinline__ bool claim_point(const uint64_t* src, uint32_t* row, const uint32_t (&gen)[16], bool& on_curve)
{
    uint32_t w[16], wx[8], wy[8];
    ld8(src, wx);
    ld8(src + 4, wy);
#pragma unroll
    for (int k = 0; k < 8; k++) { w[k] = wx[k]; w[8 + k] = wy[k]; }
    const bool inf = (wy[7] >> 31) != 0;
    AffineV<2> a;
    load_affine_m256(a, w);
    const FeT<Fq> one = fe_one<Fq>();
    const auto three = add(add(one, one), one);
    const auto d = mul_sub(a.y, a.y, sqr(a.x), a.x); // (y^2 - x^3) R
    on_curve = inf || is_zero_mulout(mul(sub(d, three), one));
    uint32_t o[16];
    store_affine_m261(o, a.x, a.y);
    uint4* q = reinterpret_cast<uint4*>(row);
#pragma unroll
    for (int k = 0; k < 4; k++)
        q[k] = make_uint4(inf ? gen[4 * k] : o[4 * k], inf ? gen[4 * k + 1] : o[4 * k + 1], inf ? gen[4 * k + 2] : o[4 * k + 2], inf ? gen[4 * k + 3] : o[4 * k + 3]);
    return inf;
}

template <bool PER_CLAIM, bool OPEN_ALL> __global__ void __launch_bounds__(CT) k_kzg_claims(KzgClaimsArgs P)
{
    __shared__ unsigned long long s_first[CT / 64];
    __shared__ uint32_t s_bad[CT / 64];
    constexpr uint64_t PER = PER_CLAIM ? 2 : 1;
    const uint64_t nt = (uint64_t)gridDim.x * blockDim.x;
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t gen[16];
    store_affine_m261(gen, fe_from<Fq>(Fq::GEN_X), fe_from<Fq>(Fq::GEN_Y));
    F2 zt = fe_one<FrP>();
    if constexpr (OPEN_ALL) { // omega^(t mod n) by square-and-multiply; from then on one product per stride
        const FeT<FrP> omega = fe_from<FrP>(P.omega.d);
        const uint32_t e = (uint32_t)t & ((1u << P.log2n) - 1u);
        for (int b = (int)P.log2n - 1; b >= 0; --b) {
            zt = sqr(zt);
            const F2 m = mul(zt, omega);
            const bool take = ((e >> b) & 1u) != 0;
#pragma unroll
            for (int i = 0; i < NL; i++) zt.d[i] = take ? m.d[i] : zt.d[i];
        }
    }
    uint32_t bad = 0;
    unsigned long long first = ~0ull;
    for (; t < P.count; t += nt) {
        uint64_t r[4];
        keccak_rho_device(P.seed, t, r);
        uint32_t rw[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { rw[2 * k] = (uint32_t)r[k]; rw[2 * k + 1] = (uint32_t)(r[k] >> 32); }
        const Fe<FrP, 1, 6> rho = unpack<FrP>(rw);
        const uint64_t row = PER * t;
        if constexpr (PER_CLAIM) {
            bool on;
            const bool inf = claim_point(P.commitments + 8 * t, P.rows + row * 16, gen, on);
            if (!on) {
                bad++;
                first = 2 * t < first ? 2 * t : first;
            }
            st8(P.scal_a + row * 4, rw, inf);
            st8(P.scal_b + row * 4, rw, true); // B does not read the commitments
        }
        bool on;
        const bool inf = claim_point(P.proofs + 8 * t, P.rows + (row + PER - 1) * 16, gen, on);
        if (!on) {
            bad++;
            first = 2 * t + 1 < first ? 2 * t + 1 : first;
        }
        uint32_t w[8], o[8];
        if constexpr (!OPEN_ALL) {
            ld8(P.z + 4 * t, w);
            zt = m256_to_m261<FrP>(unpack<FrP>(w));
        }
        to_canonical(mul(zt, rho), o);
        st8(P.scal_a + (row + PER - 1) * 4, o, inf);
        st8(P.scal_b + (row + PER - 1) * 4, rw, inf);
        ld8(P.y + 4 * t, w);
        to_canonical(mul(m256_to_m261<FrP>(unpack<FrP>(w)), rho), o);
        st8(P.term_y + 4 * t, o, false);
        if constexpr (!PER_CLAIM) st8(P.term_rho + 4 * t, rw, false);
        if constexpr (OPEN_ALL) zt = mul(zt, fe_from<FrP>(P.step.d));
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        bad += __shfl_xor(bad, o);
        const uint32_t lo = __shfl_xor((uint32_t)first, o), hi = __shfl_xor((uint32_t)(first >> 32), o);
        const unsigned long long f = ((unsigned long long)hi << 32) | lo;
        first = f < first ? f : first;
    }
    if ((threadIdx.x & 63) == 0) {
        s_bad[threadIdx.x >> 6] = bad;
        s_first[threadIdx.x >> 6] = first;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 1; k < CT / 64; k++) {
        bad += s_bad[k];
        first = s_first[k] < first ? s_first[k] : first;
    }
    if (!bad) return;
    atomicAdd(&P.find->bad_points, (unsigned long long)bad);
    atomicMin(&P.find->first_key, first);
}

// ---- k_kzg_fold: the sums over the claims t < m, one workgroup per (range of claims, slot) -----------------------------------------------------------------
// Slot k < S: sum of rho_t over the claims labelled k (which[t], or t >> log2n in the open-all form); slot S: sum of rho_t y_t over all of them.  A claim
// of another commitment costs its label, not the 32-byte term.  Canonical additions modulo r (fr_sum_device.hpp) in a fixed tree: exact, so ranges and
// tree give the value any other order would.  With one range the workgroup writes the scalar itself; with more it writes a partial sum, and
// k_kzg_fold_finish adds the ranges up the same way.
__device__ __forceinline__ void tree_sum(uint64_t (&s_acc)[CT][4], const uint64_t (&acc)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) s_acc[threadIdx.x][i] = acc[i];
    __syncthreads();
    for (uint32_t o = CT / 2; o; o >>= 1) {
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
}
// thread 0: the scalar of slot k from the sum in s_acc[0] -- on G the negated sum, on a commitment at infinity (a stand-in row) zero
__device__ __forceinline__ void put_slot(const uint64_t (&s)[4], uint32_t k, uint32_t S, unsigned long long skip_mask, uint64_t* __restrict__ out)
{
    uint64_t v[4] = { s[0], s[1], s[2], s[3] };
    if (k == S && (v[0] | v[1] | v[2] | v[3]) != 0) { // r - sum: canonical, since 0 < sum < r
        uint64_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint64_t d = FrP::P64[i] - v[i];
            const uint64_t b1 = FrP::P64[i] < v[i];
            v[i] = d - borrow;
            borrow = b1 | (uint64_t)(d < borrow);
        }
    }
    const bool skip = k < S && ((skip_mask >> k) & 1ull) != 0;
    ulonglong2* o2 = reinterpret_cast<ulonglong2*>(out + 4 * (size_t)k);
    o2[0] = make_ulonglong2(skip ? 0 : v[0], skip ? 0 : v[1]);
    o2[1] = make_ulonglong2(skip ? 0 : v[2], skip ? 0 : v[3]);
}
struct KzgFoldArgs {
    const uint64_t *term_y, *term_rho;
    const uint32_t* which; // null: the label is t >> log2n
    uint32_t log2n, S;
    uint32_t m, chunk;     // range p is the claims [p chunk, min(m, (p + 1) chunk))
    unsigned long long skip_mask;
    uint64_t* partial;     // [slot][range] x 4 words (more than one range)
    uint64_t* out;         // the first S + 1 scalars of A
};
__global__ void __launch_bounds__(CT) k_kzg_fold(KzgFoldArgs P)
{
    __shared__ uint64_t s_acc[CT][4];
    const uint32_t p = blockIdx.x, k = blockIdx.y;
    const uint32_t lo = p * P.chunk, hi = min(P.m, lo + P.chunk); // lo < m <= 2^20: no overflow
    uint64_t acc[4] = { 0, 0, 0, 0 };
    for (uint32_t t = lo + threadIdx.x; t < hi; t += CT) {
        if (k < P.S) {
            const uint32_t label = P.which ? P.which[t] : t >> P.log2n;
            if (label != k) continue;
        }
        uint64_t v[4];
        ld4((k < P.S ? P.term_rho : P.term_y) + 4 * (size_t)t, v);
        fr_add_canonical(acc, v);
    }
    tree_sum(s_acc, acc);
    if (threadIdx.x != 0) return;
    const uint64_t s[4] = { s_acc[0][0], s_acc[0][1], s_acc[0][2], s_acc[0][3] };
    if (gridDim.x == 1) {
        put_slot(s, k, P.S, P.skip_mask, P.out);
    } else {
        ulonglong2* o2 = reinterpret_cast<ulonglong2*>(P.partial + 4 * ((size_t)k * gridDim.x + p));
        o2[0] = make_ulonglong2(s[0], s[1]);
        o2[1] = make_ulonglong2(s[2], s[3]);
    }
}
// one workgroup per slot over its `ranges` <= CT partial sums
__global__ void __launch_bounds__(CT) k_kzg_fold_finish(const uint64_t* __restrict__ partial, uint32_t ranges, uint32_t S, unsigned long long skip_mask,
                                                        uint64_t* __restrict__ out)
{
    __shared__ uint64_t s_acc[CT][4];
    const uint32_t k = blockIdx.x;
    uint64_t acc[4] = { 0, 0, 0, 0 };
    if (threadIdx.x < ranges) ld4(partial + 4 * ((size_t)k * ranges + threadIdx.x), acc);
    tree_sum(s_acc, acc);
    if (threadIdx.x != 0) return;
    const uint64_t s[4] = { s_acc[0][0], s_acc[0][1], s_acc[0][2], s_acc[0][3] };
    put_slot(s, k, S, skip_mask, out);
}

} // namespace

uint32_t kzg_check_claim_threads(size_t count)
{
    return (uint32_t)std::min<size_t>((count + CT - 1) / CT, 2048) * CT; // the rest by the stride
}
uint32_t kzg_check_fold_ranges(size_t m)
{
    return (uint32_t)std::min<size_t>((m + KZG_FOLD_RANGE - 1) / KZG_FOLD_RANGE, KZG_FOLD_MAX_RANGES);
}

// B.find: one KzgFindings the caller has initialised ({0, ~0}); omega / step: read in the open-all form only, step = omega^kzg_check_claim_threads(count)
int kzg_check_claims(const KzgCheckBuffers& B, const uint64_t seed[4], size_t count, bool per_claim, bool open_all, int log2n, const uint32_t omega_m261[9],
                     const uint32_t step_m261[9], hipStream_t st)
{
    KzgClaimsArgs P{};
    P.proofs = B.proofs;
    P.commitments = B.commitments;
    P.z = B.z;
    P.y = B.y;
    P.rows = B.rows;
    P.scal_a = B.scal_a;
    P.scal_b = B.scal_b;
    P.term_y = B.term_y;
    P.term_rho = B.term_rho;
    P.find = B.find;
    P.count = count;
    P.log2n = (uint32_t)log2n;
    for (int i = 0; i < NL; i++) {
        P.omega.d[i] = open_all ? omega_m261[i] : 0;
        P.step.d[i] = open_all ? step_m261[i] : 0;
    }
    for (int k = 0; k < 4; k++) P.seed.d[k] = seed[k];
    const uint32_t blocks = kzg_check_claim_threads(count) / CT;
    if (per_claim) k_kzg_claims<true, false><<<blocks, CT, 0, st>>>(P);
    else if (open_all) k_kzg_claims<false, true><<<blocks, CT, 0, st>>>(P);
    else k_kzg_claims<false, false><<<blocks, CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// the scalars of the head of A over the claims [0, m): d_out[c] for the S shared commitments, d_out[S] on G
int kzg_check_fold(const KzgCheckBuffers& B, size_t m, size_t S, int log2n, uint64_t skip_mask, uint64_t* d_out, hipStream_t st)
{
    KzgFoldArgs P{};
    P.term_y = B.term_y;
    P.term_rho = B.term_rho;
    P.which = B.which;
    P.log2n = (uint32_t)log2n;
    P.S = (uint32_t)S;
    P.m = (uint32_t)m;
    const uint32_t ranges = kzg_check_fold_ranges(m);
    P.chunk = (uint32_t)(((m + ranges - 1) / ranges + CT - 1) / CT * CT);
    P.skip_mask = skip_mask;
    P.partial = B.partial;
    P.out = d_out;
    k_kzg_fold<<<dim3(ranges, (uint32_t)S + 1), CT, 0, st>>>(P);
    if (ranges > 1) k_kzg_fold_finish<<<(uint32_t)S + 1, CT, 0, st>>>(B.partial, ranges, (uint32_t)S, skip_mask, d_out);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
