// fr_columns.hip -- the device part of bbgpu_fr_ntt_columns_device and bbgpu_fr_recover_columns_device (include/bbgpu.h; the drivers are in capi.hip):
// transforms and the erasure decoder DOWN THE COLUMNS of a resident row-major matrix of field elements (host_fr_columns.hpp states both).  The codewords are
// short (rows <= 2048) and there may be millions of them, so a workgroup owns a tile of C = 2048 / rows whole columns and the entire decode of the tile runs
// in LDS between one load and one store:
//   k_fr_cols_tables  once per call: the twiddles rho^k and rho^-k (k < rows / 2), the shifts g^j and g^-j (j < rows) and, per set s and row i, rows^-1
//                     z_(s,i) and rows^-1 / z'_(s,i), all as Montgomery-261 multipliers in 12-word entries (nine 29-bit limbs, three 16-byte loads: load_tw of
//                     ntt.hip).  The elements stay in the memory format (Montgomery-256) from load to store, as in ntt.hip: a product with a Montgomery-261
//                     multiplier leaves them there;
//   k_fr_cols_decode  <true>: load-and-scale, IFFT, shift, FFT, division, IFFT, unshift with the verdict, FFT, store of the missing rows.  <false> is the same
//                     text with the scaling, the verdict and the row skipping compiled out: one transform, every row stored (bbgpu_fr_ntt_columns_device).
// z and z' are g1_recover.hip's (k_g1_roots, k_g1_vanish_cols: "column" read as "set") and the inversion of z' poly.hip's; neither is touched.
//
// The tile.  Element (row i, column c) of the tile is word i C + c of each of nine limb planes of 2048 words (limb-major, the column fastest): lanes that
// differ in the column index touch consecutive words.  The four transforms need NO permutation pass: the inverse transforms run decimation in frequency
// (natural order in, bit-reversed out), the forward ones decimation in time (bit-reversed in, natural out), and the pointwise passes between them index
// their tables by bitrev(i) where the data is bit-reversed.  Bank behaviour (ds_read_b32 / ds_write_b32, one word per lane and limb):
//   load, store, pointwise   lane e of a sweep touches word e: consecutive, conflict-free;
//   a stage of half h        butterfly u = (position, column) touches words i0 C + c and (i0 + h) C + c with i0 = group 2 h + position: a wave covers runs of
//                            h C consecutive words 2 h C apart -- conflict-free where h C >= 64 (every stage for rows <= 32), and where h C < 64 the wave's 64
//                            words lie in a span of 128, two lanes per bank more than the ideal: 2-way, in the log2(64 / C) stages of smallest h.  At rows =
//                            2048 (C = 1) that is six of eleven stages per transform; its cost was not measured on its own (the whole kernel: include/bbgpu.h);
//   the transform entry      <false> places row i at slot bitrev(i) while loading (one transform cannot end natural otherwise): where C < 64 a wave writes
//                            64 / C rows whose slots are multiples of rows C / (64 / C) words apart, up to 64 / C lanes per bank in that one sweep.
// Global memory: a row segment of the tile is C x 32 contiguous bytes.  From rows = 1024 on that is 64 or 32 bytes, narrower than a 128-byte line; tiles
// with neighbouring blockIdx.x share the line through L2.  That is accepted; what it costs against a wider tile (two passes) was not measured.
// Value bounds (fe.hpp tracks them in the type; a stage loop cannot, so assume_bound states them and this is the proof).  Every transform starts from
// products, < 3 p (the transform entry: unpack(), < 6 p).  Decimation in time: t = w y < 2 p, outputs x + t and x - t + 3 p: at most + 3 p per stage, <= 6 + 33
// = 39 p after eleven.  Decimation in frequency: (x - y) w < 3 p always, x + y doubles: with inputs < 3 p the bound before stage t is 3 2^(t mod 5) p <= 48 p,
// and the stages with t mod 5 == 4 bring their sum, < 96 p, down to < 3 p by reduce_value (half a butterfly's lanes, about sixty instructions: twice per
// transform at rows = 2048).  LDS elements are below FC_VMAX p = 52 p throughout.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "fr_mem_device.hpp"
#include "host_fr.hpp"

namespace bbgpu {

namespace {

constexpr int FT = 256;           // threads per workgroup of the table kernel
constexpr int FC_THREADS = 512;   // of the tile kernel: two sweeps per stage
constexpr int FC_LOG_ELEMS = 11;  // a tile is 2048 elements: C = 2048 / rows columns x rows
constexpr int FC_ELEMS = 1 << FC_LOG_ELEMS;
constexpr int FC_VMAX = 52;
constexpr int FC_TW = 12;         // words per table entry
using FrL = Fe<FrP, 1, FC_VMAX>;  // an element in LDS
using FrM = Fe<FrP, 1, 3>;        // a table entry: exact limbs, < 3 p
static_assert(FC_LOG_ELEMS == 11 && BBGPU_FR_COLUMNS_MAX_ROWS == 1u << FC_LOG_ELEMS, "one column of the largest size fills a tile");

// proof obligation is the caller's: the true bounds are <= (L, V)
template <int L, int V, int L2, int V2> __device__ __forceinline__ Fe<FrP, L, V> assume_bound(const Fe<FrP, L2, V2>& a)
{
    Fe<FrP, L, V> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.d[i] = a.d[i];
    return r;
}
__device__ __forceinline__ FrM load_mult(const uint32_t* __restrict__ table, uint32_t idx)
{
    const uint4* q = reinterpret_cast<const uint4*>(table + FC_TW * (size_t)idx);
    const uint4 a = q[0], b = q[1], c = q[2];
    FrM r;
    r.d[0] = a.x; r.d[1] = a.y; r.d[2] = a.z; r.d[3] = a.w;
    r.d[4] = b.x; r.d[5] = b.y; r.d[6] = b.z; r.d[7] = b.w;
    r.d[8] = c.x;
    return r;
}
template <int V> __device__ __forceinline__ void store_mult(uint32_t* table, uint32_t idx, const Fe<FrP, 1, V>& product) // V <= 3, exact limbs
{
    static_assert(V <= 3, "a table entry is a fresh product");
    uint4* q = reinterpret_cast<uint4*>(table + FC_TW * (size_t)idx);
    q[0] = make_uint4(product.d[0], product.d[1], product.d[2], product.d[3]);
    q[1] = make_uint4(product.d[4], product.d[5], product.d[6], product.d[7]);
    q[2] = make_uint4(product.d[8], 0, 0, 0);
}
__device__ __forceinline__ FrL lds_load(const uint32_t* lds, uint32_t pos)
{
    FrL x;
#pragma unroll
    for (int l = 0; l < NL; l++) x.d[l] = lds[l * FC_ELEMS + pos];
    return x;
}
__device__ __forceinline__ void lds_store(uint32_t* lds, uint32_t pos, const FrL& x)
{
#pragma unroll
    for (int l = 0; l < NL; l++) lds[l * FC_ELEMS + pos] = x.d[l];
}
__device__ __forceinline__ uint32_t bitrev(uint32_t x, uint32_t bits) // bits >= 1
{
    return __brev(x) >> (32 - bits);
}

// ---- k_fr_cols_tables: lane u writes entry u of every table that has one ----------------------------------------------------------------------------------
// z holds z_(s,i) as a Montgomery-261 multiplier and zci 1 / z'_(s,i) as one (k_g1_vanish_cols and the batch inversion behind it), `entries` = sets x rows of
// each, 0 for the transform entry.  A product with rows^-1 in Montgomery-261 form leaves Montgomery-261 multipliers with rows^-1 folded in, once for each of
// the decoder's two inverse transforms.  The powers by square-and-multiply over a lane-independent number of bits.
struct FrColsTableArgs {
    const uint64_t *z, *zci;
    uint32_t *tw, *twi, *kg, *kgi, *kz, *kq;
    uint32_t rows, log2rows, entries;
    Limbs9 rho, rhoinv, g, ginv, ninv;
};
__global__ void __launch_bounds__(FT) k_fr_cols_tables(FrColsTableArgs P)
{
    const uint32_t u = blockIdx.x * (uint32_t)FT + threadIdx.x;
    if (u < P.entries) {
        const FeT<FrP> ninv = fe_from<FrP>(P.ninv.d);
        uint32_t w[8];
        ld8(P.z + 4 * (size_t)u, w);
        store_mult(P.kz, u, mul(unpack<FrP>(w), ninv));
        ld8(P.zci + 4 * (size_t)u, w);
        store_mult(P.kq, u, mul(unpack<FrP>(w), ninv));
    }
    if (u < P.rows) {
        store_mult(P.kg, u, pow_bits(fe_from<FrP>(P.g.d), u, (int)P.log2rows));
        store_mult(P.kgi, u, pow_bits(fe_from<FrP>(P.ginv.d), u, (int)P.log2rows));
    }
    if (u < P.rows / 2) {
        store_mult(P.tw, u, pow_bits(fe_from<FrP>(P.rho.d), u, (int)P.log2rows - 1));
        store_mult(P.twi, u, pow_bits(fe_from<FrP>(P.rhoinv.d), u, (int)P.log2rows - 1));
    }
}

// ---- the two transforms of a tile in LDS: 1024 butterflies per stage, lane u is column u mod C of butterfly u / C ---------------------------------------------
// Stage of half h = 2^s: butterfly bf = (group, position) pairs the rows i0 = group 2 h + position and i0 + h; its twiddle is entry position (rows / 2 h).
// Both end with the barrier behind their last stage.
// decimation in time: bit-reversed in, natural out; inputs < 6 p
__device__ __forceinline__ void tile_dit(uint32_t* lds, const uint32_t* __restrict__ tw, uint32_t lg, uint32_t lgC)
{
    const uint32_t cmask = (1u << lgC) - 1;
    for (uint32_t s = 0; s < lg; s++) {
        const uint32_t half = 1u << s;
        for (uint32_t u = threadIdx.x; u < FC_ELEMS / 2; u += FC_THREADS) {
            const uint32_t c = u & cmask, bf = u >> lgC, pos = bf & (half - 1);
            const uint32_t lo = (((((bf >> s) << (s + 1)) | pos)) << lgC) | c, hi = lo + (half << lgC); // hi < rows C = 2048
            const FrL x = lds_load(lds, lo), y = lds_load(lds, hi);
            const auto t = mul(load_mult(tw, pos << (lg - 1 - s)), y); // < 2 p, exact limbs
            lds_store(lds, lo, assume_bound<1, FC_VMAX>(weak(add(x, t))));
            lds_store(lds, hi, assume_bound<1, FC_VMAX>(weak(sub(x, exact_limbs(t)))));
        }
        __syncthreads();
    }
}
// decimation in frequency: natural in, bit-reversed out; inputs < 3 p
__device__ __forceinline__ void tile_dif(uint32_t* lds, const uint32_t* __restrict__ tw, uint32_t lg, uint32_t lgC)
{
    const uint32_t cmask = (1u << lgC) - 1;
    for (uint32_t t = 0; t < lg; t++) {
        const uint32_t s = lg - 1 - t, half = 1u << s;
        const bool reduce = t % 5 == 4; // uniform
        for (uint32_t u = threadIdx.x; u < FC_ELEMS / 2; u += FC_THREADS) {
            const uint32_t c = u & cmask, bf = u >> lgC, pos = bf & (half - 1);
            const uint32_t lo = (((((bf >> s) << (s + 1)) | pos)) << lgC) | c, hi = lo + (half << lgC);
            const FrL x = lds_load(lds, lo), y = lds_load(lds, hi);
            const auto sum = add(x, y);
            const auto prod = mul(sub(x, y), load_mult(tw, pos << t)); // limbs up to 4 U into the multiplier; < 3 p
            FrL xs;
            if (reduce) xs = reduce_value(sum);
            else xs = assume_bound<1, FC_VMAX>(weak(sum)); // < 2 x 24 p
            lds_store(lds, lo, xs);
            lds_store(lds, hi, prod);
        }
        __syncthreads();
    }
}

// ---- k_fr_cols_decode ---------------------------------------------------------------------------------------------------------------------------------
// Workgroup blockIdx.x owns the columns [j0, j0 + C), j0 = blockIdx.x C, of which wc = min(C, width - j0) exist; the others stay zero in LDS, run through
// the transforms as zeros, and are neither read nor written in memory, as are the elements at [width, stride) of every row.  Column j belongs to set
// j mod sets (any sets: one integer division per element of the three sweeps that need it).  present: bit s rows + i is set where set s lists row i.
// DECODE: missing rows are not read -- their slots start at zero -- and only they are stored; the verdict is a zero test of the exact-limb product D_j for
// every j >= d, its smallest index per column met in LDS by an atomic minimum that only a NONZERO coefficient issues, so an honest call issues none; after
// the last barrier lane c writes column c's finding to bad[] (if the caller wants the per-column array) and, again only for a finding, lowers the call's
// two 64-bit keys (column << 32 | index) in memory.
struct FrColsArgs {
    uint64_t* m;                              // the matrix
    size_t stride;                            // elements between two rows
    uint32_t width, log2rows, sets, d;
    const uint32_t *tw, *twi, *kg, *kgi, *kz, *kq; // <false>: tw alone, the table of the direction asked for
    const uint32_t *moff, *present;           // sets + 1 offsets of the missing rows; the bits
    uint32_t* bad;                            // null or width
    unsigned long long* find;                 // [0] the smallest key in [d, count_s), [1] in [count_s, rows); the caller starts both at ~0
    Limbs9 scale;                             // <false>: rows^-1, Montgomery-261
    uint32_t scaled;                          // <false>: apply it (the inverse)
};
template <bool DECODE> __global__ void __launch_bounds__(FC_THREADS) k_fr_cols_decode(FrColsArgs A)
{
    extern __shared__ uint32_t lds[]; // [9][2048]; DECODE: then s_bad[C], s_bug[C]
    const uint32_t lg = A.log2rows, rows = 1u << lg, lgC = FC_LOG_ELEMS - lg, C = 1u << lgC, tid = threadIdx.x;
    const uint32_t j0 = blockIdx.x << lgC;        // < width <= 2^27
    const uint32_t wc = min(C, A.width - j0);     // >= 1
    uint32_t *s_bad = lds + NL * FC_ELEMS, *s_bug = s_bad + C;
    if constexpr (DECODE)
        for (uint32_t c = tid; c < C; c += FC_THREADS) s_bad[c] = s_bug[c] = ~0u; // read after the barriers of three transforms

    // ---- load (DECODE: scale by rows^-1 z; else the optional rows^-1), row segments of wc x 32 contiguous bytes
    for (uint32_t e = tid; e < FC_ELEMS; e += FC_THREADS) {
        const uint32_t c = e & (C - 1), i = e >> lgC;
        bool take = c < wc;
        uint32_t entry = 0;
        if constexpr (DECODE) {
            if (take) {
                entry = ((j0 + c) % A.sets) * rows + i; // < sets rows <= 2^20
                take = (A.present[entry >> 5] >> (entry & 31)) & 1u;
            }
        }
        FrL x = fe_zero<FrP>();
        if (take) {
            uint32_t w[8];
            ld8(A.m + 4 * ((size_t)i * A.stride + j0 + c), w); // i < rows, j0 + c < width <= stride
            if constexpr (DECODE) x = mul(unpack<FrP>(w), load_mult(A.kz, entry));
            else if (A.scaled) x = mul(unpack<FrP>(w), fe_from<FrP>(A.scale.d));
            else x = unpack<FrP>(w);
        }
        lds_store(lds, DECODE ? e : (bitrev(i, lg) << lgC) | c, x);
    }
    __syncthreads();

    if constexpr (DECODE) {
        tile_dif(lds, A.twi, lg, lgC); // P, bit-reversed
        for (uint32_t e = tid; e < FC_ELEMS; e += FC_THREADS) // g^j P_j
            lds_store(lds, e, mul(lds_load(lds, e), load_mult(A.kg, bitrev(e >> lgC, lg))));
        __syncthreads();
        tile_dit(lds, A.tw, lg, lgC); // Q, natural
        for (uint32_t e = tid; e < FC_ELEMS; e += FC_THREADS) { // Q_i / (rows z'_i)
            const uint32_t c = e & (C - 1), i = e >> lgC;
            lds_store(lds, e, mul(lds_load(lds, e), load_mult(A.kq, ((j0 + c) % A.sets) * rows + i))); // a column past the width: zeros times a valid entry
        }
        __syncthreads();
        tile_dif(lds, A.twi, lg, lgC); // D', bit-reversed
        for (uint32_t e = tid; e < FC_ELEMS; e += FC_THREADS) { // D_j = g^-j D'_j, and the verdict
            const uint32_t c = e & (C - 1), j = bitrev(e >> lgC, lg);
            const auto D = mul(lds_load(lds, e), load_mult(A.kgi, j)); // exact limbs, < 2 p
            lds_store(lds, e, D);
            if (j >= A.d && c < wc && !is_zero_mulout(D)) {
                const uint32_t s = (j0 + c) % A.sets, count = rows - (A.moff[s + 1] - A.moff[s]);
                if (j < count) atomicMin(&s_bad[c], j);
                else atomicMin(&s_bug[c], j);
            }
        }
        __syncthreads();
    }
    tile_dit(lds, A.tw, lg, lgC); // V, natural

    // ---- store (DECODE: the missing rows only), canonical
    for (uint32_t e = tid; e < FC_ELEMS; e += FC_THREADS) {
        const uint32_t c = e & (C - 1), i = e >> lgC;
        bool put = c < wc;
        if constexpr (DECODE) {
            if (put) {
                const uint32_t entry = ((j0 + c) % A.sets) * rows + i;
                put = !((A.present[entry >> 5] >> (entry & 31)) & 1u);
            }
        }
        if (!put) continue;
        uint32_t w[8];
        to_canonical(reduce_value(lds_load(lds, e)), w);
        st8(A.m + 4 * ((size_t)i * A.stride + j0 + c), w, false);
    }
    if constexpr (DECODE) {
        for (uint32_t c = tid; c < wc; c += FC_THREADS) {
            const uint32_t bad = s_bad[c], bug = s_bug[c];
            if (A.bad) A.bad[j0 + c] = bad;
            if (bad != ~0u) atomicMin(&A.find[0], ((unsigned long long)(j0 + c) << 32) | bad);
            if (bug != ~0u) atomicMin(&A.find[1], ((unsigned long long)(j0 + c) << 32) | bug);
        }
    }
}

constexpr size_t FC_TILE_BYTES = (size_t)NL * FC_ELEMS * 4; // 73,728
constexpr size_t FC_FIND_BYTES = 2 * 1024 * 4;              // s_bad and s_bug at C = 1024
template <bool DECODE> hipError_t launch_tile(const FrColsArgs& A, hipStream_t st)
{
    static bool attr_set = false;
    if (!attr_set) { // above the 64 KiB a kernel gets unasked: two workgroups per CU, 2 x 81,920 = 163,840 bytes, all there is
        (void)hipFuncSetAttribute((const void*)k_fr_cols_decode<DECODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(FC_TILE_BYTES + FC_FIND_BYTES));
        attr_set = true;
    }
    const uint32_t lgC = FC_LOG_ELEMS - A.log2rows, tiles = (A.width + (1u << lgC) - 1) >> lgC; // <= 2^17
    k_fr_cols_decode<DECODE><<<tiles, FC_THREADS, FC_TILE_BYTES + (DECODE ? (size_t)8 << lgC : 0), st>>>(A);
    return launch_check();
}

// the six tables in one buffer, in words from its start
struct TableLayout {
    size_t tw, twi, kg, kgi, kz, kq, words;
    TableLayout(int log2rows, size_t entries)
    {
        const size_t rows = (size_t)1 << log2rows;
        tw = 0;
        twi = tw + FC_TW * (rows / 2);
        kg = twi + FC_TW * (rows / 2);
        kgi = kg + FC_TW * rows;
        kz = kgi + FC_TW * rows;
        kq = kz + FC_TW * entries;
        words = kq + FC_TW * entries;
    }
};

} // namespace

// every function below enqueues on st and synchronises nothing; rows = 2^log2rows, 1 <= log2rows <= 11, rows x width <= 2^28

size_t fr_cols_table_words(int log2rows, size_t entries)
{
    return TableLayout(log2rows, entries).words;
}

int fr_cols_tables(const uint64_t* d_z, const uint64_t* d_zci, size_t entries, int log2rows, uint32_t* d_tabs, hipStream_t st)
{
    const TableLayout L(log2rows, entries);
    const host::Fr rho = host::fr_root_of_unity(log2rows), g = host::fr_from_limbs(FrHostP::GEN5);
    FrColsTableArgs P{};
    P.z = d_z;
    P.zci = d_zci;
    P.tw = d_tabs + L.tw;
    P.twi = d_tabs + L.twi;
    P.kg = d_tabs + L.kg;
    P.kgi = d_tabs + L.kgi;
    P.kz = d_tabs + L.kz;
    P.kq = d_tabs + L.kq;
    P.rows = 1u << log2rows;
    P.log2rows = (uint32_t)log2rows;
    P.entries = (uint32_t)entries;
    P.rho = host::limbs_m261(rho);
    P.rhoinv = host::limbs_m261(host::fr_inv(rho));
    P.g = host::limbs_m261(g);
    P.ginv = host::limbs_m261(host::fr_inv(g));
    P.ninv = host::limbs_m261(host::fr_inv(host::fr_from_u64((uint64_t)1 << log2rows)));
    k_fr_cols_tables<<<blocks_of((uint32_t)std::max<size_t>(entries, P.rows), FT), FT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

int fr_cols_transform(uint64_t* d_rows, size_t width, size_t stride_elems, int log2rows, bool inverse, const uint32_t* d_tabs, hipStream_t st)
{
    const TableLayout L(log2rows, 0);
    FrColsArgs A{};
    A.m = d_rows;
    A.stride = stride_elems;
    A.width = (uint32_t)width;
    A.log2rows = (uint32_t)log2rows;
    A.tw = d_tabs + (inverse ? L.twi : L.tw);
    A.scale = host::limbs_m261(host::fr_inv(host::fr_from_u64((uint64_t)1 << log2rows)));
    A.scaled = inverse ? 1u : 0u;
    HIPCHK(launch_tile<false>(A, st));
    return BBGPU_OK;
}

int fr_cols_decode(uint64_t* d_rows, size_t width, size_t stride_elems, int log2rows, int sets, size_t degree_bound, const uint32_t* d_tabs,
                   const uint32_t* d_moff, const uint32_t* d_present, uint32_t* d_bad, unsigned long long* d_find, hipStream_t st)
{
    const TableLayout L(log2rows, (size_t)sets << log2rows);
    FrColsArgs A{};
    A.m = d_rows;
    A.stride = stride_elems;
    A.width = (uint32_t)width;
    A.log2rows = (uint32_t)log2rows;
    A.sets = (uint32_t)sets;
    A.d = (uint32_t)degree_bound;
    A.tw = d_tabs + L.tw;
    A.twi = d_tabs + L.twi;
    A.kg = d_tabs + L.kg;
    A.kgi = d_tabs + L.kgi;
    A.kz = d_tabs + L.kz;
    A.kq = d_tabs + L.kq;
    A.moff = d_moff;
    A.present = d_present;
    A.bad = d_bad;
    A.find = d_find;
    HIPCHK(launch_tile<true>(A, st));
    return BBGPU_OK;
}

} // namespace bbgpu
