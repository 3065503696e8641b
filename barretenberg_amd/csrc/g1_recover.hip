// g1_recover.hip -- the device part of bbgpu_g1_ntt and bbgpu_g1_recover (include/bbgpu.h; the drivers are in capi.hip): transforms whose elements are curve
// points, batched over many SHORT columns, and the erasure decoder built from them (host_g1_recover.hpp states it).  A column is n scratch points (XYZZ,
// 128 bytes each, ZZ == 0 for infinity; g1_ladder.hpp), column b at slot b n of a scratch; a call owns TWO scratches and every permuting pass reads one and
// writes the other, so that no pass meets the race between a slot and its bit-reversed partner:
//   k_g1_load        slot bitrev(i) of column b <- k_i * P_(b, i) from the caller's affine points (the reference's memory format); k_i from a table, or one
//                    scalar for all, or none (the forward transform); a row that is not listed, or a point at infinity, gives infinity;
//   k_g1_stage_cols  log2 n launches per transform, in place: the butterfly of g1_stage.hpp with (position, column, group) flattened into ONE lane index.  The
//                    drivers launch it for n <= 64 and k_lagrange_stage, the column in blockIdx.y, from n = 128 on, where it measured no better
//                    (profiles/g1_recover.txt; capi.hip g1_transform_dispatch);
//   k_g1_scale       slot bitrev(j) of the other scratch <- k_j * slot j: the coset shift, the division and the unshift, each with the bit reversal of the
//                    transform behind it folded in;
//   k_g1_scalars     the four tables of per-index scalars as plain canonical integers, once per call: n^-1 z_i, g^j, n^-1 / z'_i, g^-j;
//   k_g1_verdict     the smallest coefficient index in [d, count) and in [count, n) whose slot is not at infinity, per column;
//   k_g1_finish      one Fermat inversion per point to the reference's affine format.
// The vanishing values z, z' are kzg_recover_cells.hip's through kzg_recover_vanish (its kernels are not touched), the inversion of z' poly.hip's.  One wave per
// workgroup of the ladder kernels, 3-bit windows and no twiddle table, as srs_lagrange.hip.  The reference has no counterpart.
// bbgpu_g1_recover_each -- every column with its own rows -- runs the same kernels in their per-column forms (a table row, a list of places and a count per
// column, through arguments whose zero or null value is the same-set form) behind two kernels of its own:
//   k_g1_roots       rho^k for every k < n, once per call;
//   k_g1_vanish_cols z and z' of every column by direct pair products over that column's missing rows, one lane per (column, index).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "fr_mem_device.hpp"
#include "g1_stage.hpp"
#include "host_fr.hpp"

namespace bbgpu {

namespace {

constexpr int FT = 256; // threads per workgroup of the kernels that run no ladder

struct Scalar256 {
    uint64_t d[4];
};

__device__ __forceinline__ void ld_scalar(const uint64_t* p, uint64_t (&k)[4])
{
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 a = q[0], b = q[1];
    k[0] = a.x; k[1] = a.y; k[2] = b.x; k[3] = b.y;
}

// ---- k_g1_stage_cols: stage s of `batch` transforms of size n = 2^log2n, lane u < batch n / 2 -----------------------------------------------------------
// k_lagrange_stage gives a column one blockIdx.y and a butterfly one lane: at n = 8 four live lanes in a wave of 64.  Here u runs over all butterflies of all
// columns.  With cg = batch x groups (column, group) pairs per position, groups = n >> (s + 1):
//   cg >= 64   position-major: pos = u / cg, then column, then group -- consecutive lanes take consecutive (column, group) pairs at ONE position, so the
//              twiddle, and the skip of the ladder at pos == 0, is wave-uniform (but for the one wave that straddles two positions where 64 does not divide cg);
//   cg <  64   consecutive positions of one group, then the groups, then the columns, as the late stages of k_lagrange_stage.
// At batch 1 both orders are k_lagrange_stage's own.  The butterfly is butterfly_slots<LAGRANGE_WB>, unchanged.
__global__ void __launch_bounds__(LT) k_g1_stage_cols(uint32_t* __restrict__ scratch, uint32_t log2n, uint32_t s, uint32_t batch, Limbs9 root261)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lgg = log2n - 1 - s, half = 1u << s, groups = 1u << lgg, cg = batch << lgg; // batch n / 2 <= 2^19
    if (u >= batch << (log2n - 1)) return;
    uint32_t pos, col, g;
    if (cg >= (uint32_t)LT) {
        pos = u / cg; // < half
        const uint32_t rem = u - pos * cg;
        col = rem >> lgg; // < batch
        g = rem & (groups - 1);
    } else {
        pos = u & (half - 1);
        const uint32_t rest = u >> s;
        g = rest & (groups - 1);
        col = rest >> lgg; // < batch: u < batch groups half
    }
    const size_t ia = ((size_t)col << log2n) + (size_t)g * 2 * half + pos, ib = ia + half; // ib <= col n + n - 1
    const uint32_t e = pos * groups;                                                       // < n / 2
    uint64_t k[4] = { 1, 0, 0, 0 };
    if (e) {
        Fe<FrP, 1, 2> w = fe_one<FrP>(), b = fe_from<FrP>(root261.d);
        for (uint32_t x = e; x; x >>= 1) {
            if (x & 1) w = mul(w, b);
            b = sqr(b);
        }
        FeT<FrP> one_raw = fe_zero<FrP>();
        one_raw.d[0] = 1;
        uint32_t kw[8];
        to_canonical(mul(w, one_raw), kw);
#pragma unroll
        for (int t = 0; t < 4; t++) k[t] = (uint64_t)kw[2 * t] | ((uint64_t)kw[2 * t + 1] << 32);
    }
    butterfly_slots<LAGRANGE_WB>(scratch + ia * 32, scratch + ib * 32, k, e == 0);
}

// ---- k_g1_load: slot bitrev(i) of column b <- k_i * (the caller's point of row i) ------------------------------------------------------------------------
// Lane u < batch n is position i = u / batch of column b = u mod batch: the lanes of a wave share a position -- one scalar, one decision about the ladder --
// wherever batch >= 64.  slot_of: null (every row is listed in order: count == n), or n entries, the place t of row i in the caller's list, ~0 for a row that
// is not listed.  tab: null (the scalar is `k` for every i; unit: it is one and no ladder runs), or n x 4 words of plain canonical integers.  The point is
// brought from the memory format to a resident row in registers and the ladder runs over that affine base.
// Per column (bbgpu_g1_recover_each): off holds the batch + 1 row offsets -- column b's points start at point off[b], t counts from there -- and slot_of and
// tab hold batch x n entries, column b's at b n; off null is the same-set form above, one row of each for all.
struct G1LoadArgs {
    const uint32_t* in; // batch x count x 16 words (per column: off[batch] x 16 words), the reference's affine format
    uint32_t* scratch;
    const uint32_t* slot_of;
    const uint64_t* tab;
    const uint32_t* off;
    Scalar256 k;
    uint32_t log2n, batch, count, unit;
};
__global__ void __launch_bounds__(LT) k_g1_load(G1LoadArgs P)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= P.batch << P.log2n) return;
    const uint32_t i = u / P.batch, b = u - i * P.batch; // i < n
    const uint32_t r = __brev(i) >> (32 - P.log2n);      // log2n >= 1; r < n
    const uint32_t e = P.off ? (b << P.log2n) + i : i;   // the entry of slot_of and of tab: < batch n <= 2^20
    const uint32_t t = P.slot_of ? P.slot_of[e] : i;
    uint32_t o[32];
#pragma unroll
    for (int q = 0; q < 32; q++) o[q] = 0;
    uint32_t* dst = P.scratch + (((size_t)b << P.log2n) + r) * 32;
    if (t == ~0u) {
        store_words32(dst, o);
        return;
    }
    uint32_t w[16];
    const size_t first = P.off ? P.off[b] : (size_t)b * P.count;
    const uint4* src = reinterpret_cast<const uint4*>(P.in + (first + t) * 16); // t < count (per column: < off[b + 1] - off[b])
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 v = src[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    if (w[15] >> 31) { // the flag of infinity
        store_words32(dst, o);
        return;
    }
    {
        AffineV<2> a;
        load_affine_m256(a, w);
        store_affine_m261(w, a.x, a.y);
    }
    Pt acc;
    bool inf = false;
    if (P.unit) {
        ladder_base(acc, w);
    } else {
        uint64_t k[4] = { P.k.d[0], P.k.d[1], P.k.d[2], P.k.d[3] };
        if (P.tab) ld_scalar(P.tab + 4 * (size_t)e, k);
        ladder_pt<LAGRANGE_WB>(w, k, acc, inf);
    }
    store_pt(o, acc, inf);
    store_words32(dst, o);
}

// ---- k_g1_scale: slot bitrev(j) of column b of dst <- k_j * slot j of column b of src; src != dst -----------------------------------------------------
// Lane order as k_g1_load.  k_j == 1 (j == 0 of the shift and of the unshift) and a slot at infinity run no ladder.  tab_stride: the entries between the
// rows of two columns in tab -- 0: one row for all (the shift, the unshift, and the division where every column misses the same rows), n: a row per column.
__global__ void __launch_bounds__(LT) k_g1_scale(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint64_t* __restrict__ tab, uint32_t log2n,
                                                 uint32_t batch, uint32_t tab_stride)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= batch << log2n) return;
    const uint32_t j = u / batch, b = u - j * batch;
    const uint32_t r = __brev(j) >> (32 - log2n);
    uint64_t k[4];
    ld_scalar(tab + 4 * ((size_t)b * tab_stride + j), k); // b tab_stride + j < batch n
    uint32_t w[32];
    load_words32(src + (((size_t)b << log2n) + j) * 32, w);
    uint32_t any = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) any |= w[16 + q];
    uint32_t* out = dst + (((size_t)b << log2n) + r) * 32;
    const bool unit = k[0] == 1 && (k[1] | k[2] | k[3]) == 0;
    if (unit || any == 0) { // the words as they stand (an infinite slot is all zero)
        store_words32(out, w);
        return;
    }
    Pt acc;
    bool inf;
    ladder_pt<LAGRANGE_WB>(w, k, acc, inf);
    uint32_t o[32];
    store_pt(o, acc, inf);
    store_words32(out, o);
}

// ---- k_g1_scalars: the four tables, n x 4 words each, plain canonical integers for the ladder ----------------------------------------------------------
// z holds z_i as a Montgomery-261 multiplier and zci 1 / z'_i as one (kzg_recover_vanish and the batch inversion behind it): a product with the PLAIN
// integer n^-1 leaves the plain integer n^-1 z_i, as k_lagrange_stage brings its twiddle down by a product with the plain one.  g^j and g^-j by
// square-and-multiply over the log2 n bits of j.  rows: 1, or the columns of bbgpu_g1_recover_each -- z, zci, kz and kq then hold rows x n entries, lane
// u < rows n entry u of each, and the first n lanes make kg and kgi as before.
struct G1ScalarArgs {
    const uint64_t *z, *zci;
    uint64_t *kz, *kg, *kq, *kgi;
    uint32_t n, log2n, rows;
    Limbs9 ninv_plain, g261, ginv261;
};
__device__ __forceinline__ void st_scalar(uint64_t* p, const uint32_t (&w)[8])
{
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    q[0] = make_ulonglong2(w[0] | ((uint64_t)w[1] << 32), w[2] | ((uint64_t)w[3] << 32));
    q[1] = make_ulonglong2(w[4] | ((uint64_t)w[5] << 32), w[6] | ((uint64_t)w[7] << 32));
}
__device__ __forceinline__ void ld_words8(const uint64_t* p, uint32_t (&w)[8])
{
    uint64_t k[4];
    ld_scalar(p, k);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        w[2 * t] = (uint32_t)k[t];
        w[2 * t + 1] = (uint32_t)(k[t] >> 32);
    }
}
__global__ void __launch_bounds__(FT) k_g1_scalars(G1ScalarArgs P)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n * P.rows) return;
    const FeT<FrP> ninv = fe_from<FrP>(P.ninv_plain.d);
    FeT<FrP> one_raw = fe_zero<FrP>();
    one_raw.d[0] = 1;
    uint32_t w[8], o[8];
    ld_words8(P.z + 4 * (size_t)i, w);
    to_canonical(mul(unpack<FrP>(w), ninv), o);
    st_scalar(P.kz + 4 * (size_t)i, o);
    ld_words8(P.zci + 4 * (size_t)i, w);
    to_canonical(mul(unpack<FrP>(w), ninv), o);
    st_scalar(P.kq + 4 * (size_t)i, o);
    if (i >= P.n) return; // the rows of the other columns: g^j and g^-j are one row for all
    Fe<FrP, 1, 2> a = fe_one<FrP>(), ai = fe_one<FrP>();
    const FeT<FrP> g = fe_from<FrP>(P.g261.d), gi = fe_from<FrP>(P.ginv261.d);
    for (int b = (int)P.log2n - 1; b >= 0; --b) { // the same trip count on every lane
        a = sqr(a);
        ai = sqr(ai);
        const Fe<FrP, 1, 2> m = mul(a, g), mi = mul(ai, gi);
        const bool take = ((i >> b) & 1u) != 0;
#pragma unroll
        for (int q = 0; q < NL; q++) {
            a.d[q] = take ? m.d[q] : a.d[q];
            ai.d[q] = take ? mi.d[q] : ai.d[q];
        }
    }
    to_canonical(mul(a, one_raw), o);
    st_scalar(P.kg + 4 * (size_t)i, o);
    to_canonical(mul(ai, one_raw), o);
    st_scalar(P.kgi + 4 * (size_t)i, o);
}

// ---- k_g1_verdict: ONE workgroup per column (blockIdx.x: there may be 2^19 columns); coefficient j lies at slot bitrev(j), where the unshift wrote it ------
// Strided over j in [d, n), at most 256 trips: only the eight ZZ words of a slot are read.  The smallest index of each kind meets on chip -- __shfl_xor,
// then LDS -- and thread 0 writes the column's two findings over the ~0 the caller put there: no atomic at all (k_recover_tail needs one per workgroup
// that found something, because several workgroups share a polynomial there).
// off: null, or the batch + 1 row offsets of bbgpu_g1_recover_each: column b has off[b + 1] - off[b] rows present (a scalar load, b is the workgroup's).
__global__ void __launch_bounds__(FT) k_g1_verdict(const uint32_t* __restrict__ scratch, RecoverFindings* __restrict__ find, uint32_t log2n, uint32_t d, uint32_t present,
                                                   const uint32_t* __restrict__ off)
{
    __shared__ uint32_t s_bad[FT / 64], s_bug[FT / 64];
    const uint32_t n = 1u << log2n, b = blockIdx.x;
    if (off) present = off[b + 1] - off[b];
    uint32_t bad = ~0u, bug = ~0u;
    for (uint32_t j = d + threadIdx.x; j < n; j += (uint32_t)FT) {
        const uint32_t r = __brev(j) >> (32 - log2n);
        const uint4* zz = reinterpret_cast<const uint4*>(scratch + (((size_t)b << log2n) + r) * 32 + 16);
        const uint4 lo = zz[0], hi = zz[1];
        if ((lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) != 0) {
            if (j < present) bad = min(bad, j);
            else bug = min(bug, j);
        }
    }
    if (!min_pair_to_thread0<FT>(bad, bug, s_bad, s_bug)) return;
    if (bad != ~0u) find[b].first_bad = bad;
    if (bug != ~0u) find[b].first_bug = bug;
}

// ---- k_g1_roots: rho^k for every k < n, once per call of bbgpu_g1_recover_each ------------------------------------------------------------------------------
// Square-and-multiply over the log2 n bits of k as k_recover_roots, the nine limbs limb-major (limb q of rho^k at roots[q n + k]) in the Montgomery-261 form
// the products of k_g1_vanish_cols take: neighbouring lanes read neighbouring words there, both for their own rho^i and when they stage a tile.
__global__ void __launch_bounds__(FT) k_g1_roots(uint32_t* __restrict__ roots, uint32_t log2n, Limbs9 rho)
{
    const uint32_t k = blockIdx.x * (uint32_t)FT + threadIdx.x, n = 1u << log2n;
    if (k >= n) return;
    const Fe<FrP, 1, 2> r = pow_bits(fe_from<FrP>(rho.d), k, (int)log2n);
#pragma unroll
    for (int q = 0; q < NL; q++) roots[(size_t)q * n + k] = r.d[q];
}

// ---- k_g1_vanish_cols: z_(b,i) = prod_{k in K_b} (rho^i - rho^k) and z'_(b,i) = prod_{k in K_b} (g rho^i - rho^k) for every column b and every i < n -------
// Lane u < batch n is index i = u mod n of column b = u / n.  The missing rows of all columns lie in ONE array, column b's (ascending) at
// missing[moff[b] .. moff[b + 1]), so the lists of neighbouring columns are neighbours.  A workgroup of FT = 256 lanes covers the columns [b0, b1): one
// column (a 256-lane part of it) where n >= 256, the 256 / n whole columns from b0 = blockIdx.x 256 / n on -- fewer at the end of the grid -- where n < 256.
// Its stretch of the array, `span` = moff[b1] - moff[b0] entries, is walked in tiles of VT = 256 roots: lane tid copies the nine limbs of the root of entry
// base + tid from k_g1_roots' table into LDS, limb-major, and after the barrier every lane runs over the part of the tile that belongs to ITS column.  At
// n >= 256 that is the whole tile on every lane (the reads are one word for the wave: a broadcast); at n < 256 the stretch holds at most (256 / n)(n - 1)
// < 256 entries, one tile, and the lanes of a wave read 64 / n different sub-ranges at n < 64.  Per (i, k) a lane reads one root and runs TWO accumulators
// over it, one subtraction and one product each.  What depends on the workgroup alone -- b0, b1, span, the tile loop and its two barriers -- is computed
// from blockIdx.x, so every lane reaches every barrier whatever its column misses; the inner loop has the lane's own bounds and no barrier in it (a column
// that misses nothing runs no trip: both values one); a lane past the end of the grid has an empty range, stages like the others and writes nothing.
// z as a Montgomery-261 multiplier and z' x 2^-5 in the memory format, the forms of k_recover_vanish: the batch inversion and k_g1_scalars follow unchanged.
constexpr int VT = KZG_RECOVER_TILE; // roots per LDS tile
static_assert(VT == FT, "k_g1_vanish_cols: lane tid stages entry tid of a tile");
struct G1VanishArgs {
    const uint32_t *roots, *moff, *missing; // n x 9 words; batch + 1; moff[batch] rows, each < n
    uint64_t *z, *zc;                       // batch x n x 4 words each
    uint32_t log2n, batch;
    Limbs9 g;    // the coset generator, Montgomery-261
    Limbs9 c251; // the plain integer 2^251 mod r
};
__global__ void __launch_bounds__(FT) k_g1_vanish_cols(G1VanishArgs P)
{
    __shared__ uint32_t s_root[NL][VT];
    using F2 = Fe<FrP, 1, 2>;
    const uint32_t tid = threadIdx.x, n = 1u << P.log2n, u = blockIdx.x * (uint32_t)FT + tid; // batch n <= 2^20
    const bool live = u < P.batch << P.log2n;
    const uint32_t b0 = (blockIdx.x * (uint32_t)FT) >> P.log2n;                          // < batch: the grid has ceil(batch n / FT) workgroups
    const uint32_t b1 = min(b0 + max(1u, (uint32_t)FT >> P.log2n), P.batch);             // <= batch
    const uint32_t g0 = P.moff[b0], span = P.moff[b1] - g0;                              // uniform over the workgroup
    const uint32_t b = live ? u >> P.log2n : b0, i = u & (n - 1u);                       // b0 <= b < b1
    const uint32_t first = live ? P.moff[b] - g0 : 0u, last = live ? P.moff[b + 1] - g0 : 0u; // first <= last <= span
    F2 x;
#pragma unroll
    for (int q = 0; q < NL; q++) x.d[q] = P.roots[(size_t)q * n + i];
    const F2 xc = mul(x, fe_from<FrP>(P.g.d));
    const FeT<FrP> one = fe_one<FrP>();
    F2 acc = one, accc = one;
    for (uint32_t base = 0; base < span; base += (uint32_t)VT) {
        const uint32_t entries = min((uint32_t)VT, span - base);
        const uint32_t k = tid < entries ? P.missing[g0 + base + tid] : 0u; // g0 + base + tid < moff[b1]; k < n
#pragma unroll
        for (int q = 0; q < NL; q++) s_root[q][tid] = tid < entries ? P.roots[(size_t)q * n + k] : 0u;
        __syncthreads();
        const uint32_t lo = max(first, base), hi = min(last, base + entries);
        for (uint32_t t = lo; t < hi; t++) { // t - base < entries <= VT
            F2 r;
#pragma unroll
            for (int q = 0; q < NL; q++) r.d[q] = s_root[q][t - base];
            acc = mul(acc, sub(x, exact_limbs(r)));
            accc = mul(accc, sub(xc, exact_limbs(r)));
        }
        __syncthreads(); // the next tile writes the roots again
    }
    if (!live) return;
    uint32_t o[8];
    to_canonical(acc, o);
    st8(P.z + 4 * (size_t)u, o, false);
    to_canonical(mul(accc, fe_from<FrP>(P.c251.d)), o);
    st8(P.zc + 4 * (size_t)u, o, false);
}

// ---- k_g1_finish: point u < total <- the affine form of slot u in the reference's format; infinity is an ordinary result (k_open_cosets_finish) ------------
__global__ void __launch_bounds__(FT) k_g1_finish(const uint32_t* __restrict__ scratch, uint32_t* __restrict__ out, uint32_t total)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= total) return;
    uint32_t w[32], o[16];
    load_words32(scratch + (size_t)u * 32, w);
    affine_from_scratch(w, o);
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)u * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) dst[t] = make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
}

} // namespace

// every function below enqueues on st and synchronises nothing; batch x n <= 2^20, n = 2^log2n, 1 <= log2n <= 16

// d_in: batch x count x 64 bytes, the caller's points; d_slot_of: null or n entries; d_tab: null or n x 4 words; k_plain: the scalar for all when d_tab is
// null, null for none (the points as they are); d_off: null, or the row offsets of the per-column form (bbgpu_internal.h; count is not read then)
int g1_cols_load(const uint32_t* d_in, size_t count, const uint32_t* d_slot_of, const uint64_t* d_tab, const uint64_t* k_plain, uint32_t* d_scratch, int log2n,
                 int batch, hipStream_t st, const uint32_t* d_off)
{
    G1LoadArgs P{};
    P.in = d_in;
    P.scratch = d_scratch;
    P.slot_of = d_slot_of;
    P.tab = d_tab;
    P.off = d_off;
    for (int i = 0; i < 4; i++) P.k.d[i] = k_plain ? k_plain[i] : 0;
    P.log2n = (uint32_t)log2n;
    P.batch = (uint32_t)batch;
    P.count = (uint32_t)count;
    P.unit = !d_tab && !k_plain;
    k_g1_load<<<blocks_of((uint32_t)batch << log2n, LT), LT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// log2 n launches of k_g1_stage_cols over the batch columns of d_scratch; root_m261: a primitive n-th root of unity or its inverse, Montgomery-261
int g1_cols_transform(uint32_t* d_scratch, int log2n, int batch, const uint32_t root_m261[9], hipStream_t st)
{
    const Limbs9 root = to_limbs9(root_m261);
    const uint32_t lanes = (uint32_t)batch << (log2n - 1);
    for (uint32_t s = 0; s < (uint32_t)log2n; s++) k_g1_stage_cols<<<blocks_of(lanes, LT), LT, 0, st>>>(d_scratch, (uint32_t)log2n, s, (uint32_t)batch, root);
    HIPCHK(launch_check()); // the chain of stages
    return BBGPU_OK;
}

// the same transforms by the mapping the other group entries use: k_lagrange_stage, the column in blockIdx.y (batch <= 65535: always so from n = 128 on,
// where the drivers choose it; bbgpu_g1_set_stage_mapping(1) asks for it at every n, for the comparison of profiles/g1_recover.txt)
int g1_cols_transform_rows(uint32_t* d_scratch, int log2n, int batch, const uint32_t root_m261[9], hipStream_t st)
{
    if (batch > 65535) {
        set_error("g1 transform, stage mapping 1: %d columns do not fit blockIdx.y", batch);
        return BBGPU_ERR_SIZE;
    }
    const Limbs9 root = to_limbs9(root_m261);
    const uint32_t n = 1u << log2n;
    for (uint32_t s = 0; s < (uint32_t)log2n; s++)
        k_lagrange_stage<<<dim3(blocks_of(n / 2, LT), (uint32_t)batch), LT, 0, st>>>(d_scratch, n, (uint32_t)log2n, s, root, (size_t)n);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

int g1_cols_scale(const uint32_t* d_src, uint32_t* d_dst, const uint64_t* d_tab, int log2n, int batch, hipStream_t st, bool per_column)
{
    k_g1_scale<<<blocks_of((uint32_t)batch << log2n, LT), LT, 0, st>>>(d_src, d_dst, d_tab, (uint32_t)log2n, (uint32_t)batch, per_column ? 1u << log2n : 0u);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_z, d_zci: kzg_recover_vanish's z and the batch inversion of its z' -> d_tabs: 4 n x 4 words, the tables kz | kg | kq | kgi; with cols > 0 (the
// per-column form: g1_cols_vanish's z and z') z, zci, kz and kq hold cols x n entries each and d_tabs (2 cols + 2) n x 4 words in the same order
int g1_cols_scalars(const uint64_t* d_z, const uint64_t* d_zci, uint64_t* d_tabs, int log2n, const uint32_t ninv_plain[9], const uint32_t g_m261[9],
                    const uint32_t ginv_m261[9], hipStream_t st, int cols)
{
    const size_t n = (size_t)1 << log2n, rows = cols > 0 ? (size_t)cols : 1;
    G1ScalarArgs P{};
    P.z = d_z;
    P.zci = d_zci;
    P.kz = d_tabs;
    P.kg = d_tabs + 4 * rows * n;
    P.kq = P.kg + 4 * n;
    P.kgi = P.kq + 4 * rows * n;
    P.n = (uint32_t)n;
    P.rows = (uint32_t)rows;
    P.log2n = (uint32_t)log2n;
    P.ninv_plain = to_limbs9(ninv_plain);
    P.g261 = to_limbs9(g_m261);
    P.ginv261 = to_limbs9(ginv_m261);
    k_g1_scalars<<<blocks_of((uint32_t)(rows * n), FT), FT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_find: batch findings, every word ~0; coefficient j of column b at slot bitrev(j); d_off: null, or the row offsets that give every column its own `present`
int g1_cols_verdict(const uint32_t* d_scratch, int log2n, int batch, size_t degree_bound, size_t present, RecoverFindings* d_find, hipStream_t st,
                    const uint32_t* d_off)
{
    const size_t n = (size_t)1 << log2n;
    if (degree_bound >= n) return BBGPU_OK; // no coefficient to look at
    k_g1_verdict<<<(uint32_t)batch, FT, 0, st>>>(d_scratch, d_find, (uint32_t)log2n, (uint32_t)degree_bound, (uint32_t)present, d_off);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// z and z' x 2^-5 of every column by direct pair products (bbgpu_internal.h): k_g1_roots, then k_g1_vanish_cols over batch x n lanes
int g1_cols_vanish(const uint32_t* d_moff, const uint32_t* d_missing, int log2n, int batch, uint32_t* d_roots, uint64_t* d_z, uint64_t* d_zc, hipStream_t st)
{
    G1VanishArgs P{};
    P.roots = d_roots;
    P.moff = d_moff;
    P.missing = d_missing;
    P.z = d_z;
    P.zc = d_zc;
    P.log2n = (uint32_t)log2n;
    P.batch = (uint32_t)batch;
    P.g = host::limbs_m261(host::fr_from_limbs(FrHostP::GEN5));
    P.c251 = host::limbs_m256(host::fr_inv(host::fr_from_u64(32))); // the limbs of the words as they stand: 2^-5 in Montgomery form IS the integer 2^251
    k_g1_roots<<<blocks_of(1u << log2n, FT), FT, 0, st>>>(d_roots, (uint32_t)log2n, host::limbs_m261(host::fr_root_of_unity(log2n)));
    k_g1_vanish_cols<<<blocks_of((uint32_t)batch << log2n, FT), FT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_out: batch x n x 64 bytes, natural order
int g1_cols_finish(const uint32_t* d_scratch, uint32_t* d_out, int log2n, int batch, hipStream_t st)
{
    const uint32_t total = (uint32_t)batch << log2n;
    k_g1_finish<<<blocks_of(total, FT), FT, 0, st>>>(d_scratch, d_out, total);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
