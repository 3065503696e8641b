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
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "fr_mem_device.hpp"
#include "g1_stage.hpp"

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
struct G1LoadArgs {
    const uint32_t* in; // batch x count x 16 words, the reference's affine format
    uint32_t* scratch;
    const uint32_t* slot_of;
    const uint64_t* tab;
    Scalar256 k;
    uint32_t log2n, batch, count, unit;
};
__global__ void __launch_bounds__(LT) k_g1_load(G1LoadArgs P)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= P.batch << P.log2n) return;
    const uint32_t i = u / P.batch, b = u - i * P.batch; // i < n
    const uint32_t r = __brev(i) >> (32 - P.log2n);      // log2n >= 1; r < n
    const uint32_t t = P.slot_of ? P.slot_of[i] : i;
    uint32_t o[32];
#pragma unroll
    for (int q = 0; q < 32; q++) o[q] = 0;
    uint32_t* dst = P.scratch + (((size_t)b << P.log2n) + r) * 32;
    if (t == ~0u) {
        store_words32(dst, o);
        return;
    }
    uint32_t w[16];
    const uint4* src = reinterpret_cast<const uint4*>(P.in + ((size_t)b * P.count + t) * 16); // t < count
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
        if (P.tab) ld_scalar(P.tab + 4 * (size_t)i, k);
        ladder_pt<LAGRANGE_WB>(w, k, acc, inf);
    }
    store_pt(o, acc, inf);
    store_words32(dst, o);
}

// ---- k_g1_scale: slot bitrev(j) of column b of dst <- k_j * slot j of column b of src; src != dst -----------------------------------------------------
// Lane order as k_g1_load.  k_j == 1 (j == 0 of the shift and of the unshift) and a slot at infinity run no ladder.
__global__ void __launch_bounds__(LT) k_g1_scale(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, const uint64_t* __restrict__ tab, uint32_t log2n,
                                                 uint32_t batch)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= batch << log2n) return;
    const uint32_t j = u / batch, b = u - j * batch;
    const uint32_t r = __brev(j) >> (32 - log2n);
    uint64_t k[4];
    ld_scalar(tab + 4 * (size_t)j, k);
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
// square-and-multiply over the log2 n bits of j.
struct G1ScalarArgs {
    const uint64_t *z, *zci;
    uint64_t *kz, *kg, *kq, *kgi;
    uint32_t n, log2n;
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
    if (i >= P.n) return;
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
__global__ void __launch_bounds__(FT) k_g1_verdict(const uint32_t* __restrict__ scratch, RecoverFindings* __restrict__ find, uint32_t log2n, uint32_t d, uint32_t present)
{
    __shared__ uint32_t s_bad[FT / 64], s_bug[FT / 64];
    const uint32_t n = 1u << log2n, b = blockIdx.x;
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
// null, null for none (the points as they are)
int g1_cols_load(const uint32_t* d_in, size_t count, const uint32_t* d_slot_of, const uint64_t* d_tab, const uint64_t* k_plain, uint32_t* d_scratch, int log2n,
                 int batch, hipStream_t st)
{
    G1LoadArgs P{};
    P.in = d_in;
    P.scratch = d_scratch;
    P.slot_of = d_slot_of;
    P.tab = d_tab;
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

int g1_cols_scale(const uint32_t* d_src, uint32_t* d_dst, const uint64_t* d_tab, int log2n, int batch, hipStream_t st)
{
    k_g1_scale<<<blocks_of((uint32_t)batch << log2n, LT), LT, 0, st>>>(d_src, d_dst, d_tab, (uint32_t)log2n, (uint32_t)batch);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_z, d_zci: kzg_recover_vanish's z and the batch inversion of its z' -> d_tabs: 4 n x 4 words, the tables kz | kg | kq | kgi
int g1_cols_scalars(const uint64_t* d_z, const uint64_t* d_zci, uint64_t* d_tabs, int log2n, const uint32_t ninv_plain[9], const uint32_t g_m261[9],
                    const uint32_t ginv_m261[9], hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    G1ScalarArgs P{};
    P.z = d_z;
    P.zci = d_zci;
    P.kz = d_tabs;
    P.kg = d_tabs + 4 * n;
    P.kq = d_tabs + 8 * n;
    P.kgi = d_tabs + 12 * n;
    P.n = (uint32_t)n;
    P.log2n = (uint32_t)log2n;
    P.ninv_plain = to_limbs9(ninv_plain);
    P.g261 = to_limbs9(g_m261);
    P.ginv261 = to_limbs9(ginv_m261);
    k_g1_scalars<<<blocks_of((uint32_t)n, FT), FT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_find: batch findings, every word ~0; coefficient j of column b at slot bitrev(j)
int g1_cols_verdict(const uint32_t* d_scratch, int log2n, int batch, size_t degree_bound, size_t present, RecoverFindings* d_find, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    if (degree_bound >= n) return BBGPU_OK; // no coefficient to look at
    k_g1_verdict<<<(uint32_t)batch, FT, 0, st>>>(d_scratch, d_find, (uint32_t)log2n, (uint32_t)degree_bound, (uint32_t)present);
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
