// kzg_recover_each.hip -- the device parts of bbgpu_kzg_recover_cells_each (include/bbgpu.h; the driver is in capi.hip) that are not a transform or the
// batch inversion: the vanishing polynomial of every polynomial's OWN missing cells in COEFFICIENT form from a product tree -- leaves of T roots, then
// levels of sibling products between two batched transforms -- its gather into the inputs of the two transforms that give its values on the domain and
// on the coset, and scatter, divide and tail with per-polynomial lists.  The definition all follow is host_kzg_recover_each.hpp's
// kzg_recover_cells_each_host (the host twin, which forms no tree).  Notation as in kzg_recover_cells.hip: l = 2^log2l values per cell, m = 2^log2m cells
// per polynomial, n = l m, psi = omega^l, g the coset generator of BBGPU_COSET_FFT, Y = X^l; polynomial b misses the mu_b cells K_b.  M is the common
// power of two >= max mu_b (at least 1, at most m) to which every polynomial's root list is padded with ZERO roots: the padded product is
// Y^(M - mu_b) Z_b, so Z_b's coefficients are read from offset M - mu_b -- exact, no division, no case for a mu_b that is no power of two.
// The 16-byte loads and stores and the square-and-multiply are restated from kzg_recover_cells.hip, and scatter, divide and tail are that file's with a
// per-polynomial base: that file's kernels keep their own, so that bbgpu_kzg_recover_cells stays what it was.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "fe.hpp"
#include "host_fr.hpp"

namespace bbgpu {

namespace {

constexpr int CT = 256;                  // threads per workgroup, every kernel here
constexpr int LT = KZG_RECOVER_EACH_LEAF; // roots per leaf: one wave, one coefficient per lane
static_assert(LT == 64 || LT == 128 || LT == 256, "k_each_leaves: a leaf is one, two or four waves of one workgroup");
using F2 = Fe<FrP, 1, 2>; // a product

__device__ __forceinline__ void ld8(const uint64_t* p, uint32_t (&w)[8])
{
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 a = q[0], b = q[1];
    w[0] = (uint32_t)a.x; w[1] = (uint32_t)(a.x >> 32); w[2] = (uint32_t)a.y; w[3] = (uint32_t)(a.y >> 32);
    w[4] = (uint32_t)b.x; w[5] = (uint32_t)(b.x >> 32); w[6] = (uint32_t)b.y; w[7] = (uint32_t)(b.y >> 32);
}
__device__ __forceinline__ void st8(uint64_t* p, const uint32_t (&w)[8], bool zero)
{
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    const uint64_t v0 = w[0] | ((uint64_t)w[1] << 32), v1 = w[2] | ((uint64_t)w[3] << 32), v2 = w[4] | ((uint64_t)w[5] << 32), v3 = w[6] | ((uint64_t)w[7] << 32);
    q[0] = make_ulonglong2(zero ? 0 : v0, zero ? 0 : v1);
    q[1] = make_ulonglong2(zero ? 0 : v2, zero ? 0 : v3);
}
// base^e over the low `bits` bits of e, most significant first: the same trip count on every lane
__device__ __forceinline__ F2 pow_bits(const FeT<FrP>& base, uint32_t e, int bits)
{
    F2 acc = fe_one<FrP>();
    for (int b = bits - 1; b >= 0; --b) {
        acc = sqr(acc);
        const F2 m = mul(acc, base);
        const bool take = ((e >> b) & 1u) != 0;
#pragma unroll
        for (int i = 0; i < NL; i++) acc.d[i] = take ? m.d[i] : acc.d[i];
    }
    return acc;
}

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

// ---- k_each_scatter, k_each_divide, k_each_tail: kzg_recover_cells.hip's, every polynomial with its own lists and its own z, z' ---------------------------
struct EachLists {
    const uint32_t *off, *mu; // batch + 1 cell offsets; batch counts of missing cells
    const uint32_t *cell, *missing; // off[batch] listed cells; batch x M missing cells (the first mu_b of a row)
    uint32_t M;
};
struct EachScatterArgs {
    const uint64_t* values; // off[batch] x l x 4
    EachLists L;
    const uint64_t* z; // batch x m x 4
    uint64_t* out;
    size_t stride;
    uint32_t log2l, log2m;
};
__global__ void __launch_bounds__(CT) k_each_scatter(EachScatterArgs P)
{
    const uint32_t u = blockIdx.x * (uint32_t)CT + threadIdx.x, b = blockIdx.y;
    if (u >= (1u << (P.log2l + P.log2m))) return;
    const uint32_t off = P.L.off[b], present = (P.L.off[b + 1] - off) << P.log2l;
    uint64_t* out = P.out + 4 * (size_t)b * P.stride;
    uint32_t o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (u < present) {
        const uint32_t k = P.L.cell[off + (u >> P.log2l)], j = u & ((1u << P.log2l) - 1u);
        uint32_t w[8], zw[8];
        ld8(P.values + 4 * (((size_t)off << P.log2l) + u), w);
        ld8(P.z + 4 * (((size_t)b << P.log2m) + k), zw);
        to_canonical(mul(unpack<FrP>(w), unpack<FrP>(zw)), o);
        st8(out + 4 * ((size_t)k + ((size_t)j << P.log2m)), o, false);
    } else {
        const uint32_t mu = P.L.mu[b], v = u - present, j = v / mu, k = P.L.missing[(size_t)b * P.L.M + (v - j * mu)]; // mu > 0 here: present < n
        st8(out + 4 * ((size_t)k + ((size_t)j << P.log2m)), o, true);
    }
}

__global__ void __launch_bounds__(CT) k_each_divide(uint64_t* __restrict__ q, size_t stride, const uint64_t* __restrict__ inv, uint32_t log2n, uint32_t log2m)
{
    const uint32_t i = blockIdx.x * (uint32_t)CT + threadIdx.x, b = blockIdx.y;
    if (i >= (1u << log2n)) return;
    uint64_t* p = q + 4 * ((size_t)b * stride + i);
    uint32_t w[8], zw[8], o[8];
    ld8(p, w);
    ld8(inv + 4 * (((size_t)b << log2m) + (i & ((1u << log2m) - 1u))), zw);
    to_canonical(mul(unpack<FrP>(w), unpack<FrP>(zw)), o);
    st8(p, o, false);
}

struct EachTailArgs {
    uint64_t *coeffs, *copy;
    size_t stride;
    const uint32_t* off;   // batch + 1
    RecoverFindings* find; // batch, the caller has set every word to ~0
    uint32_t log2n, log2l, d;
};
__global__ void __launch_bounds__(CT) k_each_tail(EachTailArgs P)
{
    __shared__ uint32_t s_bad[CT / 64], s_bug[CT / 64];
    const uint32_t n = 1u << P.log2n, b = blockIdx.y, present = (P.off[b + 1] - P.off[b]) << P.log2l;
    const FeT<FrP> one = fe_one<FrP>();
    uint32_t bad = ~0u, bug = ~0u;
    for (uint32_t i = blockIdx.x * (uint32_t)CT + threadIdx.x; i < n; i += gridDim.x * (uint32_t)CT) {
        uint64_t* p = P.coeffs + 4 * ((size_t)b * P.stride + i);
        uint32_t w[8], o[8];
        ld8(p, w);
        to_canonical(mul(unpack<FrP>(w), one), o);
        st8(p, o, false);
        if (P.copy) st8(P.copy + 4 * (((size_t)b << P.log2n) + i), o, false);
        const bool nz = (o[0] | o[1] | o[2] | o[3] | o[4] | o[5] | o[6] | o[7]) != 0;
        if (nz && i >= P.d) {
            if (i < present) bad = min(bad, i);
            else bug = min(bug, i);
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        bad = min(bad, (uint32_t)__shfl_xor((int)bad, o));
        bug = min(bug, (uint32_t)__shfl_xor((int)bug, o));
    }
    if ((threadIdx.x & 63) == 0) {
        s_bad[threadIdx.x >> 6] = bad;
        s_bug[threadIdx.x >> 6] = bug;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 1; k < CT / 64; k++) {
        bad = min(bad, s_bad[k]);
        bug = min(bug, s_bug[k]);
    }
    if (bad != ~0u) atomicMin(&P.find[b].first_bad, (unsigned long long)bad);
    if (bug != ~0u) atomicMin(&P.find[b].first_bug, (unsigned long long)bug);
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

static EachLists each_lists(const KzgRecoverEachLists& L)
{
    EachLists R{};
    R.off = L.d_off;
    R.mu = L.d_mu;
    R.cell = L.d_cell;
    R.missing = L.d_missing;
    R.M = (uint32_t)L.M;
    return R;
}

// d_values: off[batch] x l x 4 words; d_z: batch x m x 4; d_out: batch polynomials, stride_elems apart
int kzg_recover_each_scatter(const uint64_t* d_values, const KzgRecoverEachLists& L, const uint64_t* d_z, int log2n, int log2l, int batch, uint64_t* d_out,
                             size_t stride_elems, hipStream_t st)
{
    EachScatterArgs P{};
    P.values = d_values;
    P.L = each_lists(L);
    P.z = d_z;
    P.out = d_out;
    P.stride = stride_elems;
    P.log2l = (uint32_t)log2l;
    P.log2m = (uint32_t)(log2n - log2l);
    const size_t n = (size_t)1 << log2n;
    k_each_scatter<<<dim3((uint32_t)((n + CT - 1) / CT), (uint32_t)batch), CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

int kzg_recover_each_divide(uint64_t* d_q, size_t stride_elems, int batch, const uint64_t* d_inv, int log2n, int log2l, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    k_each_divide<<<dim3((uint32_t)((n + CT - 1) / CT), (uint32_t)batch), CT, 0, st>>>(d_q, stride_elems, d_inv, (uint32_t)log2n, (uint32_t)(log2n - log2l));
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_find: batch findings, every word ~0; d_copy: null or batch x n x 4 words
int kzg_recover_each_tail(uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* d_copy, int log2n, int log2l, size_t degree_bound, const uint32_t* d_off,
                          RecoverFindings* d_find, hipStream_t st)
{
    EachTailArgs P{};
    P.coeffs = d_coeffs;
    P.copy = d_copy;
    P.stride = stride_elems;
    P.off = d_off;
    P.find = d_find;
    P.log2n = (uint32_t)log2n;
    P.log2l = (uint32_t)log2l;
    P.d = (uint32_t)degree_bound;
    const size_t n = (size_t)1 << log2n;
    const uint32_t blocks = (uint32_t)std::min<size_t>((n + CT - 1) / CT, KZG_RECOVER_TAIL_MAX_BLOCKS);
    k_each_tail<<<dim3(blocks, (uint32_t)batch), CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
