// kzg_recover_each.hip -- the device parts of bbgpu_kzg_recover_cells_each (include/bbgpu.h; the driver is in capi.hip) that are not a transform or the
// batch inversion: the vanishing polynomial of every polynomial's OWN missing cells in COEFFICIENT form from a product tree -- leaves of T roots, then
// levels of sibling products between two batched transforms -- its gather into the inputs of the two transforms that give its values on the domain and
// on the coset.  The definition all follow is host_kzg_recover_each.hpp's
// kzg_recover_cells_each_host (the host twin, which forms no tree).  Notation as in kzg_recover_cells.hip: l = 2^log2l values per cell, m = 2^log2m cells
// per polynomial, n = l m, psi = omega^l, g the coset generator of BBGPU_COSET_FFT, Y = X^l; polynomial b misses the mu_b cells K_b.  M is the common
// power of two >= max mu_b (at least 1, at most m) to which every polynomial's root list is padded with ZERO roots: the padded product is
// Y^(M - mu_b) Z_b, so Z_b's coefficients are read from offset M - mu_b -- exact, no division, no case for a mu_b that is no power of two.
// Scatter, divide and tail are kzg_recover_cells.hip's, which take per-polynomial lists (RecoverLists, bbgpu_internal.h); the 16-byte loads and stores
// and the square-and-multiply are fr_mem_device.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "fe.hpp"
#include "fr_mem_device.hpp"
#include "host_fr.hpp"

namespace bbgpu {

namespace {

constexpr int CT = 256;                  // threads per workgroup, every kernel here
constexpr int LT = KZG_RECOVER_EACH_LEAF; // roots per leaf: one wave, one coefficient per lane
static_assert(LT == 64 || LT == 128 || LT == 256, "k_each_leaves: a leaf is one, two or four waves of one workgroup");
using F2 = Fe<FrP, 1, 2>; // a product

// ---- k_each_leaves: T = min(LT, M) roots -> the T low coefficients of prod (Y - r), the leading 1 implied ---------------------------------------------
// One coefficient per lane: a leaf is max(1, T / 64) neighbouring WAVES of a workgroup of CT / 64, one wave in the build that ships (LT = 64; LT = 256,
// the other figure of include/bbgpu.h, is a build with KZG_RECOVER_EACH_LEAF = 256).  Leaf t of the call (polynomial t / (M / T), its roots t T .. t T
// + T of the padded list) goes to slot t of 2 T elements: coefficients in the low half, zeros in the high half.  Thread i of a leaf first computes
// -psi^(K[i]) by square-and-multiply (0 for a padding entry, ~0 in the list) into LDS, limb-major, so that the loop reads root k as nine broadcast
// words.  The polynomial is held TOP-ALIGNED: after k roots thread i holds the coefficient of Y^(i - (T - k)), threads below T - k hold zero and the
// leading 1 sits, implied, at thread T.  Multiplying by (Y - r) then is   c_i <- c_i - r c_(i+1)   with c_T = 1: the neighbour's nine limbs by
// __shfl_down -- across a wave boundary through LDS, lane 0 of every wave posting its limbs before ONE barrier per root, in two buffers by turns (a wave
// can post root k + 2 only after every wave has passed the barrier of root k + 1, that is after every read of root k) -- and one mul_add (c_i x 1 + (-r)
// x c_(i+1) under one reduction, which keeps the bound of c at that of a product) per lane and root; after T roots thread i holds coefficient i.  A zero
// root leaves every lane as it is: the product by Y is the shift that the alignment has already made.  The trip count T is the same on every lane and no
// lane leaves before the last barrier; lanes at or above T (M < 64 only) and waves past the last leaf compute on zeros and write nothing.
struct EachLeavesArgs {
    const uint32_t* missing; // batch x M: the missing cells of polynomial b, then ~0
    uint64_t* tree;          // leaves x 2 T x 4 words
    uint32_t leaves, T, log2m;
    Limbs9 psi; // Montgomery-261
};
__global__ void __launch_bounds__(CT) k_each_leaves(EachLeavesArgs P)
{
    __shared__ uint32_t s_root[NL][CT];
    __shared__ uint32_t s_edge[2][CT / 64][NL];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t wpl = P.T > 64u ? P.T >> 6 : 1u;                 // waves per leaf
    const uint32_t first = w - (w & (wpl - 1u));                    // the leaf's first wave in this workgroup
    const uint32_t i_of = ((w - first) << 6) + lane;                // this thread's coefficient
    const uint32_t leaf = (blockIdx.x * (uint32_t)(CT / 64) + first) / wpl;
    const bool live = leaf < P.leaves && i_of < P.T;
    const uint32_t k = live ? P.missing[(size_t)leaf * P.T + i_of] : ~0u;
    {
        const F2 r = pow_bits(fe_from<FrP>(P.psi.d), k == ~0u ? 0u : k, (int)P.log2m);
        const Fe<FrP, 1, 3> nr = weak(neg(r));
#pragma unroll
        for (int q = 0; q < NL; q++) s_root[q][tid] = k == ~0u ? 0u : nr.d[q];
    }
    __syncthreads();
    const FeT<FrP> one = fe_one<FrP>();
    const bool across = LT > 64 && wpl > 1u, from_next = across && lane == 63u && w + 1u < first + wpl;
    F2 c = fe_zero<FrP>();
    for (uint32_t i = 0; i < P.T; i++) {
        if constexpr (LT > 64) {
            if (across) { // uniform over the workgroup
                if (lane == 0u) {
#pragma unroll
                    for (int q = 0; q < NL; q++) s_edge[i & 1u][w][q] = c.d[q];
                }
                __syncthreads();
            }
        }
        Fe<FrP, 1, 3> nr;
        F2 cn;
#pragma unroll
        for (int q = 0; q < NL; q++) {
            nr.d[q] = s_root[q][(first << 6) + i];
            uint32_t up = (uint32_t)__shfl_down((int)c.d[q], 1);
            if constexpr (LT > 64) up = from_next ? s_edge[i & 1u][(w + 1u) & (uint32_t)(CT / 64 - 1)][q] : up;
            cn.d[q] = i_of == P.T - 1u ? one.d[q] : up;
        }
        c = mul_add(c, one, nr, cn);
    }
    if (!live) return;
    uint32_t o[8];
    to_canonical(m261_to_m256<FrP>(c), o);
    uint64_t* slot = P.tree + 4 * ((size_t)leaf * 2u * P.T);
    st8(slot + 4 * (size_t)i_of, o, false);
    st8(slot + 4 * (size_t)(P.T + i_of), o, true);
}

// ---- k_each_pair: the values of a sibling pair's product, between the two transforms of a level -----------------------------------------------------------
// A node of a level is X^D + a, its slot of 2 D elements holds the transform of a (size 2 D, natural order).  (X^D + a)(X^D + b) = X^(2D) + X^D (a + b)
// + a b with deg a b <= 2 D - 2: the low part X^D (a + b) + a b has degree < 2 D, so the cyclic transform of size 2 D holds it WITHOUT wrap-around, and
// at the point w^j, where X^D = (-1)^j, its value is   s (A_j + B_j) + A_j B_j,   s = (-1)^j.   Thread (pair p, point j) writes that over A_j -- the
// inverse transform of slot 2 p, at stride 4 D, then gives the 2 D low coefficients of the parent in the low half of ITS slot of 4 D elements -- and zero
// over B_j, the high half of that slot.  Every thread reads and writes its own two elements only.  Two products per point: A into Montgomery-261, then
// times B.
__global__ void __launch_bounds__(CT) k_each_pair(uint64_t* __restrict__ tree, uint32_t log2s /* log2 (2 D) */, uint32_t points /* pairs x 2 D */)
{
    const uint32_t u = blockIdx.x * (uint32_t)CT + threadIdx.x;
    if (u >= points) return;
    const uint32_t j = u & ((1u << log2s) - 1u), p = u >> log2s;
    uint64_t *pa = tree + 4 * ((((size_t)2 * p) << log2s) + j), *pb = pa + ((size_t)4 << log2s);
    uint32_t wa[8], wb[8], o[8];
    ld8(pa, wa);
    ld8(pb, wb);
    const auto A = unpack<FrP>(wa), B = unpack<FrP>(wb);
    const F2 ab = mul(m256_to_m261<FrP>(A), B);
    const auto sum = add(A, B);
    const auto nsum = neg(sum);
    Fe<FrP, 4, 13> t;
#pragma unroll
    for (int q = 0; q < NL; q++) t.d[q] = (j & 1u) ? nsum.d[q] : sum.d[q];
    to_canonical(add(ab, t), o);
    st8(pa, o, false);
    st8(pb, o, true);
}

// ---- k_each_powers: (g^l)^j in two tables, j = lo + (hi << lo_bits); the high table carries the factor 2^-5 ------------------------------------------------
__global__ void __launch_bounds__(CT) k_each_powers(uint32_t* __restrict__ tab, uint32_t lo_bits, uint32_t hi_bits, Limbs9 gl, Limbs9 gl_hi, Limbs9 factor)
{
    const uint32_t i = blockIdx.x * (uint32_t)CT + threadIdx.x, nlo = 1u << lo_bits, nhi = 1u << hi_bits;
    if (i >= nlo + nhi) return;
    const bool hi = i >= nlo;
    F2 r = pow_bits(fe_from<FrP>(hi ? gl_hi.d : gl.d), hi ? i - nlo : i, (int)(hi ? hi_bits : lo_bits));
    const F2 scaled = mul(r, fe_from<FrP>(factor.d));
#pragma unroll
    for (int q = 0; q < NL; q++) tab[(size_t)i * NL + q] = hi ? scaled.d[q] : r.d[q];
}

// ---- k_each_gather: coefficient j < m of Z_b (blockIdx.y = b), times 2^5 into zin, times (g^l)^j 2^-5 into zcin ------------------------------------------
// Z_b's coefficient j is the padded product's coefficient j + M - mu_b for j < mu_b, the implied 1 at j = mu_b, zero above.  The transform of zin is z_a
// as a Montgomery-261 multiplier, that of zcin is z'_a x 2^-5 in the memory format: what k_recover_vanish writes (see there for what the inversion makes
// of it).  mu_b = 0: Z_b = 1.
struct EachGatherArgs {
    const uint64_t* tree; // batch slots of 2 M elements
    const uint32_t* mu;   // batch
    const uint32_t* tab;  // k_each_powers
    uint64_t *zin, *zcin; // batch x m x 4 words each
    uint32_t m, M, lo_bits;
    Limbs9 c32, one256; // 32 in Montgomery-261; the integer 2^256 mod r
};
__global__ void __launch_bounds__(CT) k_each_gather(EachGatherArgs P)
{
    const uint32_t j = blockIdx.x * (uint32_t)CT + threadIdx.x, b = blockIdx.y;
    if (j >= P.m) return;
    const uint32_t mu = P.mu[b];
    uint64_t *pz = P.zin + 4 * ((size_t)b * P.m + j), *pzc = P.zcin + 4 * ((size_t)b * P.m + j);
    uint32_t o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (j > mu) {
        st8(pz, o, true);
        st8(pzc, o, true);
        return;
    }
    Fe<FrP, 1, 6> c = fe_from<FrP>(P.one256.d);
    if (j < mu) {
        uint32_t w[8];
        ld8(P.tree + 4 * ((size_t)b * 2u * P.M + (P.M - mu) + j), w);
        c = unpack<FrP>(w);
    }
    to_canonical(mul(c, fe_from<FrP>(P.c32.d)), o);
    st8(pz, o, false);
    F2 lo, hi;
#pragma unroll
    for (int q = 0; q < NL; q++) {
        lo.d[q] = P.tab[(size_t)(j & ((1u << P.lo_bits) - 1u)) * NL + q];
        hi.d[q] = P.tab[((size_t)(1u << P.lo_bits) + (j >> P.lo_bits)) * NL + q];
    }
    to_canonical(mul(mul(c, lo), hi), o);
    st8(pzc, o, false);
}

} // namespace

// d_missing: batch x M cells, polynomial b's mu_b missing cells first, then ~0 -> d_tree: batch M / T leaves, T = min(LT, M), in slots of 2 T elements
int kzg_recover_each_leaves(const uint32_t* d_missing, int batch, size_t M, int log2m, uint64_t* d_tree, hipStream_t st)
{
    EachLeavesArgs P{};
    P.missing = d_missing;
    P.tree = d_tree;
    P.T = (uint32_t)std::min<size_t>(LT, M);
    P.leaves = (uint32_t)((size_t)batch * M / P.T);
    P.log2m = (uint32_t)log2m;
    P.psi = host::limbs_m261(host::fr_root_of_unity(log2m));
    const uint32_t per = (uint32_t)CT / std::max(64u, P.T); // leaves per workgroup
    k_each_leaves<<<(P.leaves + per - 1) / per, CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// between the forward and the inverse transform of a level: `pairs` sibling pairs of slots of 2^log2s elements
int kzg_recover_each_pair(uint64_t* d_tree, size_t pairs, int log2s, hipStream_t st)
{
    const size_t points = pairs << log2s; // batch x M at most: 2^22
    k_each_pair<<<(uint32_t)((points + CT - 1) / CT), CT, 0, st>>>(d_tree, (uint32_t)log2s, (uint32_t)points);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_tree: batch slots of 2 M elements, the padded products; d_mu: batch; d_tab: kzg_recover_each_table_words(log2m) words of workspace -> d_zin, d_zcin:
// batch x m x 4 words each, the inputs of the two size-m transforms
int kzg_recover_each_gather(const uint64_t* d_tree, const uint32_t* d_mu, int batch, size_t M, int log2n, int log2l, uint32_t* d_tab, uint64_t* d_zin,
                            uint64_t* d_zcin, hipStream_t st)
{
    const int log2m = log2n - log2l, lo_bits = (log2m + 1) / 2, hi_bits = log2m - lo_bits;
    host::Fr gl = host::fr_from_limbs(FrHostP::GEN5);
    for (int i = 0; i < log2l; i++) gl = host::fr_sqr(gl);
    host::Fr gl_hi = gl;
    for (int i = 0; i < lo_bits; i++) gl_hi = host::fr_sqr(gl_hi);
    const uint32_t entries = (1u << lo_bits) + (1u << hi_bits);
    k_each_powers<<<(entries + CT - 1) / CT, CT, 0, st>>>(d_tab, (uint32_t)lo_bits, (uint32_t)hi_bits, host::limbs_m261(gl), host::limbs_m261(gl_hi),
                                                         host::limbs_m261(host::fr_inv(host::fr_from_u64(32))));
    EachGatherArgs P{};
    P.tree = d_tree;
    P.mu = d_mu;
    P.tab = d_tab;
    P.zin = d_zin;
    P.zcin = d_zcin;
    P.m = 1u << log2m;
    P.M = (uint32_t)M;
    P.lo_bits = (uint32_t)lo_bits;
    P.c32 = host::limbs_m261(host::fr_from_u64(32));
    P.one256 = host::limbs_m256(host::fr_one());
    k_each_gather<<<dim3((P.m + CT - 1) / CT, (uint32_t)batch), CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
