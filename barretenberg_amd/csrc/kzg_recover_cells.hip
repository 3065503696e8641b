// kzg_recover_cells.hip -- the device parts of bbgpu_kzg_recover_cells (include/bbgpu.h; the driver is in capi.hip) that are not a transform or the batch
// inversion: the values of the vanishing polynomial of the missing cells, the scatter of the present cells times those values, the division on the coset
// and the tail that canonicalises the coefficients and looks for the ones that must be zero.  The definition all follow is
// host_kzg_recover_cells.hpp's kzg_recover_cells_host (the host twin).  The reference has no recovery.  Notation: l = 2^log2l values per cell, m =
// 2^log2m cells per polynomial, n = l m, psi = omega^l the m-th root, K the mu missing cells (ascending), g the coset generator of BBGPU_COSET_FFT.
// Scatter, divide and tail are also the back end of bbgpu_kzg_recover_cells_each (kzg_recover_each.hip has what only that entry needs): they read every
// polynomial's lists through RecoverLists (bbgpu_internal.h).  The 16-byte loads and stores, the square-and-multiply and the workgroup minimum of the
// findings are fr_mem_device.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "fe.hpp"
#include "fr_mem_device.hpp"
#include "host_fr.hpp"

namespace bbgpu {

namespace {

constexpr int CT = 256; // threads per workgroup, every kernel here
constexpr int RT = KZG_RECOVER_TILE; // roots per LDS tile of k_recover_vanish
static_assert(RT == CT, "k_recover_vanish: thread tid stages root tid of a tile");
using F2 = Fe<FrP, 1, 2>; // a product

// ---- k_recover_roots: psi^k for every missing cell k, once per call -------------------------------------------------------------------------------------
// Thread i takes K[i]: square-and-multiply over the log2 m bits of the index, the nine limbs of the product written limb-major (limb q of root i at
// roots[q mu + i]) in the Montgomery-261 form the products of k_recover_vanish take, so that a workgroup there reads a tile limb by limb in a row.
__global__ void __launch_bounds__(CT) k_recover_roots(const uint32_t* __restrict__ missing, uint32_t* __restrict__ roots, uint32_t mu, uint32_t log2m, Limbs9 psi)
{
    const uint32_t i = blockIdx.x * (uint32_t)CT + threadIdx.x;
    if (i >= mu) return;
    const F2 r = pow_bits(fe_from<FrP>(psi.d), missing[i], (int)log2m);
#pragma unroll
    for (int q = 0; q < NL; q++) roots[(size_t)q * mu + i] = r.d[q];
}

// ---- k_recover_vanish: z_a = prod_{k in K} (psi^a - psi^k) and z'_a = prod_{k in K} (g^l psi^a - psi^k) for every a < m -----------------------------------
// G = 2^log2g NEIGHBOURING LANES PER a: thread tid of a workgroup is slice s = tid mod G of a = (blockIdx.x CT + tid) / G, so a wave holds 64 / G whole
// groups.  G = 1 gives one a per lane; the launcher widens G when m alone would not fill the device (kzg_recover_group_log2).  The workgroup walks K in
// tiles of RT roots: thread tid copies the nine limbs of root base + tid from k_recover_roots' array into LDS, limb-major; after the barrier slice s
// takes entries s, s + G, .. of the tile.  The roots come from a kernel of their own because a tile's roots computed HERE cost every thread 2 log2 m products
// per tile beside the 2 RT / G a lane spends on its pairs -- 28 beside 32 at m = 2^14, G = 16, and that form of the kernel took 1.88 times the time of
// its product count at the rate of fe_mont_gfx950.h against 1.2 for this one (profiles/kzg_recover_cells.txt has both).
// Per (a, k) a lane reads one root -- the lanes of a group read neighbouring words, lanes of the same slice the same word: no bank conflict -- and runs TWO accumulators over it, one subtraction and one product each, independent of one
// another.  The trip count of a tile, ceil(entries / G), is the same on every lane of the workgroup: a lane whose entry lies past the end of K
// multiplies by one, a lane whose a lies past m computes a = 0 and writes nothing, so every lane reaches every barrier and every exchange.  The G
// partial products then meet in a complete tree across lanes by __shfl_xor (groups never straddle a wave), both accumulators at every level, and slice 0
// writes z_a as a Montgomery-261 multiplier for k_recover_scatter and z'_a x 2^-5 in the memory format: the batch inversion of poly.hip then returns
// 1 / z'_a x 2^5, the Montgomery-261 multiplier k_recover_divide wants.  psi^a by square-and-multiply, g^l psi^a by one more product.  mu = 0: no tile,
// every value one.
struct RecoverVanishArgs {
    const uint32_t* roots; // 9 x mu words: k_recover_roots (never read when mu == 0)
    uint64_t *z, *zc;      // m x 4 words each, canonical
    uint32_t m, log2m, mu, log2g;
    Limbs9 psi, gl; // Montgomery-261
    Limbs9 c251;    // the plain integer 2^251 mod r
};
__global__ void __launch_bounds__(CT) k_recover_vanish(RecoverVanishArgs P)
{
    __shared__ uint32_t s_root[NL][RT];
    const uint32_t tid = threadIdx.x, G = 1u << P.log2g, s = tid & (G - 1u);
    const uint32_t a_of = (blockIdx.x * (uint32_t)CT + tid) >> P.log2g;
    const bool live = a_of < P.m;
    const uint32_t a = live ? a_of : 0u;
    const FeT<FrP> psi = fe_from<FrP>(P.psi.d);
    const F2 x = pow_bits(psi, a, (int)P.log2m), xc = mul(x, fe_from<FrP>(P.gl.d));
    const FeT<FrP> one = fe_one<FrP>();
    F2 acc = one, accc = one;
    for (uint32_t base = 0; base < P.mu; base += RT) {
        const uint32_t entries = min((uint32_t)RT, P.mu - base);
#pragma unroll
        for (int q = 0; q < NL; q++) s_root[q][tid] = tid < entries ? P.roots[(size_t)q * P.mu + base + tid] : 0u;
        __syncthreads();
        const uint32_t trips = (entries + G - 1u) >> P.log2g; // s + G (trips - 1) < RT: G divides RT
        for (uint32_t t = 0; t < trips; t++) {
            const uint32_t i = s + (t << P.log2g);
            const bool has = i < entries;
            F2 r;
#pragma unroll
            for (int q = 0; q < NL; q++) r.d[q] = s_root[q][i];
            auto d = sub(x, exact_limbs(r)), dc = sub(xc, exact_limbs(r));
#pragma unroll
            for (int q = 0; q < NL; q++) {
                d.d[q] = has ? d.d[q] : one.d[q];
                dc.d[q] = has ? dc.d[q] : one.d[q];
            }
            acc = mul(acc, d);
            accc = mul(accc, dc);
        }
        __syncthreads(); // the next tile writes the roots again
    }
    for (uint32_t o = G >> 1; o; o >>= 1) {
        F2 p, pc;
#pragma unroll
        for (int q = 0; q < NL; q++) {
            p.d[q] = (uint32_t)__shfl_xor((int)acc.d[q], (int)o);
            pc.d[q] = (uint32_t)__shfl_xor((int)accc.d[q], (int)o);
        }
        acc = mul(acc, p);
        accc = mul(accc, pc);
    }
    if (!live || s != 0) return;
    uint32_t o[8];
    to_canonical(acc, o);
    st8(P.z + 4 * (size_t)a, o, false);
    to_canonical(mul(accc, fe_from<FrP>(P.c251.d)), o);
    st8(P.zc + 4 * (size_t)a, o, false);
}

// ---- k_recover_scatter, k_recover_divide, k_recover_tail: the back end of BOTH entries, polynomial b = blockIdx.y by the lists of RecoverLists --------------
// b is uniform over a workgroup, so what a thread reads per polynomial -- off[b], off[b + 1], mu[b] -- is a scalar load.  The same-set entry is the case
// in which every polynomial shares one row: off[b] = b count, which places its values; a mask of zero on the offset into `cell`, and a stride of zero
// between the rows of `missing` and between the z (and z') of two polynomials.

// ---- k_recover_scatter: E of polynomial b, every slot of [0, n) written once ---------------------------------------------------------------------------
// With count_b = off[b + 1] - off[b] listed cells: thread u < count_b l takes value j = u mod l of listed cell t = u / l -- the lanes of a wave read 2 KiB
// in a row -- and writes v z_(cell[t]), canonical, to slot cell[t] + m j; thread count_b l + u' writes the zero of point j = u' / mu_b of missing cell
// K_b[u' mod mu_b] (neighbouring lanes neighbouring missing cells).  The writes of a cell lie m elements apart, 32 bytes each.  Not transposed through
// LDS: the pass moves 2 x 32 bytes per element once per call beside three transforms that move each element log2 n / 4 or more times.
struct RecoverScatterArgs {
    const uint64_t* values; // off[batch] x l x 4
    RecoverLists L;
    const uint64_t* z; // m x 4 per polynomial, L.z_stride elements apart
    uint64_t* out;
    size_t stride;
    uint32_t log2l, log2m;
};
__global__ void __launch_bounds__(CT) k_recover_scatter(RecoverScatterArgs P)
{
    const uint32_t u = blockIdx.x * (uint32_t)CT + threadIdx.x, b = blockIdx.y;
    if (u >= (1u << (P.log2l + P.log2m))) return;
    const uint32_t off = P.L.d_off[b], present = (P.L.d_off[b + 1] - off) << P.log2l;
    uint64_t* out = P.out + 4 * (size_t)b * P.stride;
    uint32_t o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (u < present) {
        const uint32_t k = P.L.d_cell[(off & P.L.cell_mask) + (u >> P.log2l)], j = u & ((1u << P.log2l) - 1u);
        uint32_t w[8], zw[8];
        ld8(P.values + 4 * (((size_t)off << P.log2l) + u), w);
        ld8(P.z + 4 * ((size_t)b * P.L.z_stride + k), zw);
        to_canonical(mul(unpack<FrP>(w), unpack<FrP>(zw)), o);
        st8(out + 4 * ((size_t)k + ((size_t)j << P.log2m)), o, false);
    } else {
        const uint32_t mu = P.L.d_mu[b], v = u - present, j = v / mu, k = P.L.d_missing[(size_t)b * P.L.missing_stride + (v - j * mu)]; // mu > 0 here: present < n
        st8(out + 4 * ((size_t)k + ((size_t)j << P.log2m)), o, true);
    }
}

// ---- k_recover_divide: Q_i *= 1 / z'_(i mod m) of polynomial b; inv holds the Montgomery-261 multipliers, z_stride elements between polynomials --------------
__global__ void __launch_bounds__(CT) k_recover_divide(uint64_t* __restrict__ q, size_t stride, const uint64_t* __restrict__ inv, uint32_t z_stride, uint32_t log2n,
                                                       uint32_t log2m)
{
    const uint32_t i = blockIdx.x * (uint32_t)CT + threadIdx.x, b = blockIdx.y;
    if (i >= (1u << log2n)) return;
    uint64_t* p = q + 4 * ((size_t)b * stride + i);
    uint32_t w[8], zw[8], o[8];
    ld8(p, w);
    ld8(inv + 4 * ((size_t)b * z_stride + (i & ((1u << log2m) - 1u))), zw);
    to_canonical(mul(unpack<FrP>(w), unpack<FrP>(zw)), o);
    st8(p, o, false);
}

// ---- k_recover_tail: coefficients [0, n) of polynomial b canonical, and the two findings ------------------------------------------------------------------
// Strided over the coefficients.  A nonzero coefficient at an index in [d, count_b l) is a finding about the DATA (first_bad), one in [count_b l, n) a
// finding about this library (first_bug); the smallest index of each meets on chip (min_pair_to_thread0) and ONE thread per workgroup issues an atomicMin
// per kind, only if the workgroup found one: an honest call issues none.  copy: null, or batch x n x 4 words that get the same coefficients (the input of
// the forward transform behind values_out).
struct RecoverTailArgs {
    uint64_t *coeffs, *copy;
    size_t stride;
    const uint32_t* off;   // batch + 1
    RecoverFindings* find; // batch, the caller has set every word to ~0
    uint32_t log2n, log2l, d;
};
__global__ void __launch_bounds__(CT) k_recover_tail(RecoverTailArgs P)
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
    if (!min_pair_to_thread0<CT>(bad, bug, s_bad, s_bug)) return;
    if (bad != ~0u) atomicMin(&P.find[b].first_bad, (unsigned long long)bad);
    if (bug != ~0u) atomicMin(&P.find[b].first_bug, (unsigned long long)bug);
}

} // namespace

// lanes per a of k_recover_vanish: 2^18 threads (four waves on every SIMD of 256 compute units) when m alone has fewer, at most one wave per a
int kzg_recover_group_log2(int log2m)
{
    return std::min(6, std::max(0, 18 - log2m));
}

// d_missing: mu cells, ascending; d_roots: 9 x mu words of workspace (neither is read when mu == 0) -> d_z, d_zc: m x 4 words each
int kzg_recover_vanish(const uint32_t* d_missing, size_t mu, int log2n, int log2l, uint32_t* d_roots, uint64_t* d_z, uint64_t* d_zc, hipStream_t st)
{
    const int log2m = log2n - log2l, log2g = kzg_recover_group_log2(log2m);
    RecoverVanishArgs P{};
    P.roots = d_roots;
    P.z = d_z;
    P.zc = d_zc;
    P.m = 1u << log2m;
    P.log2m = (uint32_t)log2m;
    P.mu = (uint32_t)mu;
    P.log2g = (uint32_t)log2g;
    host::Fr gl = host::fr_from_limbs(FrHostP::GEN5);
    for (int i = 0; i < log2l; i++) gl = host::fr_sqr(gl);
    P.psi = host::limbs_m261(host::fr_root_of_unity(log2m));
    P.gl = host::limbs_m261(gl);
    P.c251 = host::limbs_m256(host::fr_inv(host::fr_from_u64(32))); // the limbs of the words as they stand: 2^-5 in Montgomery form IS the integer 2^251
    const size_t threads = (size_t)P.m << log2g;
    if (mu) k_recover_roots<<<(uint32_t)((mu + CT - 1) / CT), CT, 0, st>>>(d_missing, d_roots, P.mu, P.log2m, P.psi);
    k_recover_vanish<<<(uint32_t)((threads + CT - 1) / CT), CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_values: off[batch] x l x 4 words; d_z: m x 4 words per polynomial; d_out: batch polynomials, stride_elems apart
int kzg_recover_scatter(const uint64_t* d_values, const RecoverLists& L, const uint64_t* d_z, int log2n, int log2l, int batch, uint64_t* d_out, size_t stride_elems,
                        hipStream_t st)
{
    RecoverScatterArgs P{};
    P.values = d_values;
    P.L = L;
    P.z = d_z;
    P.out = d_out;
    P.stride = stride_elems;
    P.log2l = (uint32_t)log2l;
    P.log2m = (uint32_t)(log2n - log2l);
    const size_t n = (size_t)1 << log2n;
    k_recover_scatter<<<dim3((uint32_t)((n + CT - 1) / CT), (uint32_t)batch), CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

int kzg_recover_divide(uint64_t* d_q, size_t stride_elems, int batch, const uint64_t* d_inv, const RecoverLists& L, int log2n, int log2l, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    k_recover_divide<<<dim3((uint32_t)((n + CT - 1) / CT), (uint32_t)batch), CT, 0, st>>>(d_q, stride_elems, d_inv, L.z_stride, (uint32_t)log2n,
                                                                                         (uint32_t)(log2n - log2l));
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_find: batch findings, every word ~0; d_copy: null or batch x n x 4 words
int kzg_recover_tail(uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* d_copy, int log2n, int log2l, size_t degree_bound, const RecoverLists& L,
                     RecoverFindings* d_find, hipStream_t st)
{
    RecoverTailArgs P{};
    P.coeffs = d_coeffs;
    P.copy = d_copy;
    P.stride = stride_elems;
    P.off = L.d_off;
    P.find = d_find;
    P.log2n = (uint32_t)log2n;
    P.log2l = (uint32_t)log2l;
    P.d = (uint32_t)degree_bound;
    const size_t n = (size_t)1 << log2n;
    const uint32_t blocks = (uint32_t)std::min<size_t>((n + CT - 1) / CT, KZG_RECOVER_TAIL_MAX_BLOCKS);
    k_recover_tail<<<dim3(blocks, (uint32_t)batch), CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
