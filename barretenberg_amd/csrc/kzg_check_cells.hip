// kzg_check_cells.hip -- the device parts of a check of KZG cell proofs (include/bbgpu.h: bbgpu_kzg_check_cells, bbgpu_kzg_check_open_cosets and the two
// _layout entries of up to 2^16 commitments, whose own kernels are the last section; one driver in capi.hip) that are not an MSM: the per-cell rows and
// scalars, the coefficients of every cell's interpolation polynomial under the random multipliers,
// and the sums over the cells of the scalars on the shared commitments and on P_0 .. P_(l-1).  The definition all follow is host_kzg_check_cells.hpp's
// kzg_cells_host (the host twin); the sums A and B are the existing device MSM over the rows and scalars written here, the pairing is host code
// (host_pairing.hpp).  The reference has no check of cell proofs.  The 16-byte loads and stores and the square-and-multiply are
// fr_mem_device.hpp's; the curve test of a claim's point and the tree of canonical additions are restated from kzg_check.hip: that file's kernels keep
// their own.
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

// A point in the reference's format: read by four 16-byte loads, tested against the curve, written as a resident row (Montgomery-261, canonical; the
// generator `gen` for the point at infinity, which then stands under scalar zero).  Returns the infinity flag; *off: finite and off the curve.  What
// k_kzg_cells does to a proof and k_kzg_layout_commitments to a commitment.
__device__ __forceinline__ bool point_to_row(const uint64_t* __restrict__ p, const uint32_t (&gen)[16], uint32_t* __restrict__ row, bool* off)
{
    uint32_t w[16], wx[8], wy[8];
    ld8(p, wx);
    ld8(p + 4, wy);
#pragma unroll
    for (int k = 0; k < 8; k++) { w[k] = wx[k]; w[8 + k] = wy[k]; }
    const bool inf = (wy[7] >> 31) != 0;
    AffineV<2> a;
    load_affine_m256(a, w);
    const FeT<Fq> one = fe_one<Fq>();
    const auto three = add(add(one, one), one);
    const auto d = mul_sub(a.y, a.y, sqr(a.x), a.x); // (y^2 - x^3) R
    *off = !(inf || is_zero_mulout(mul(sub(d, three), one)));
    uint32_t o[16];
    store_affine_m261(o, a.x, a.y);
    uint4* q = reinterpret_cast<uint4*>(row);
#pragma unroll
    for (int k = 0; k < 4; k++)
        q[k] = make_uint4(inf ? gen[4 * k] : o[4 * k], inf ? gen[4 * k + 1] : o[4 * k + 1], inf ? gen[4 * k + 2] : o[4 * k + 2], inf ? gen[4 * k + 3] : o[4 * k + 3]);
    return inf;
}

// ---- k_kzg_cells: ONE CELL PER THREAD, strided -------------------------------------------------------------------------------------------------------------
// What k_kzg_claims<false, false> does per claim, for a cell: one Keccak permutation (rho_t, kept for the coefficient kernel and the fold), the curve
// test of pi_t and its resident row (the generator under scalar zero for infinity), the scalars rho_t psi^(k_t) for A -- psi^(k_t) by square-and-multiply
// over the log2 m bits of k_t, the product with rho_t READ AS AN INTEGER, exactly the twin's fr_mul(psi^k, rho) -- and rho_t for B.  Findings meet on chip
// and ONE thread per workgroup issues the two atomics, only if the workgroup found anything: an honest call issues none.  Key of a finding: 2 t + 1.
struct KzgCellsArgs {
    const uint64_t* proofs;
    const uint32_t* cell; // null: k_t = t mod m
    uint32_t* rows;
    uint64_t *scal_a, *scal_b, *term_rho;
    KzgFindings* find;
    uint64_t count;
    uint32_t log2m;
    Limbs9 psi; // Montgomery-261
    Seed seed;
};
__global__ void __launch_bounds__(CT) k_kzg_cells(KzgCellsArgs P)
{
    __shared__ unsigned long long s_first[CT / 64];
    __shared__ uint32_t s_bad[CT / 64];
    const uint64_t nt = (uint64_t)gridDim.x * blockDim.x;
    uint32_t gen[16];
    store_affine_m261(gen, fe_from<Fq>(Fq::GEN_X), fe_from<Fq>(Fq::GEN_Y));
    const FeT<FrP> psi = fe_from<FrP>(P.psi.d);
    uint32_t bad = 0;
    unsigned long long first = ~0ull;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < P.count; t += nt) {
        uint64_t r[4];
        keccak_rho_device(P.seed, t, r);
        uint32_t rw[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { rw[2 * k] = (uint32_t)r[k]; rw[2 * k + 1] = (uint32_t)(r[k] >> 32); }
        const Fe<FrP, 1, 6> rho = unpack<FrP>(rw);
        // pi_t: read, tested, written as a row
        bool off;
        const bool inf = point_to_row(P.proofs + 8 * t, gen, P.rows + t * 16, &off);
        if (off) {
            bad++;
            first = 2 * t + 1 < first ? 2 * t + 1 : first;
        }
        const uint32_t k = P.cell ? P.cell[t] : (uint32_t)t & ((1u << P.log2m) - 1u);
        uint32_t s[8];
        to_canonical(mul(pow_bits(psi, k, (int)P.log2m), rho), s);
        st8(P.scal_a + 4 * t, s, inf);
        st8(P.scal_b + 4 * t, rw, inf);
        st8(P.term_rho + 4 * t, rw, false);
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

// ---- k_kzg_cell_coefficients: l NEIGHBOURING LANES PER CELL, strided over cells ----------------------------------------------------------------------------
// Thread tid of a workgroup is lane j = tid mod l of the cell base + tid / l: a wave holds 64 / l whole cells, a workgroup C = 256 / l, and the stride
// loop runs over workgroup-uniform bases, so every lane of every wave -- those of a cell past the end included, which compute on zeros and write nothing --
// reaches every barrier and every exchange.  A lane
//   1. holds one value: in the labelled form its own 32 bytes (the lanes of a wave read 2 KiB in a row); in the open-cosets form the values of a cell lie
//      m elements apart, so the workgroup loads TRANSPOSED -- thread tid reads value tid / C of cell base + tid mod C, neighbouring threads neighbouring
//      cells, C x 32 bytes in a row -- and hands the words over through 8 KiB of LDS;
//   2. brings it into the field and divides by l in ONE product (x 2^5 / l in Montgomery-261 form: memory form -> Montgomery-261);
//   3. runs the log2 l decimation-in-frequency stages of the size-l inverse transform across lanes: the partner's nine limbs by __shfl_xor (cells never
//      straddle a wave), then ONE product per lane and stage -- the lower lane (u + v) x 1, the upper (u - v) x zeta^(-q 2^s), both with the same limb
//      bounds -- with roots from the table of l <= 64 entries that came with the head; lane j ends up with coefficient i = bitreverse(j);
//   4. multiplies by the twist omega^(-k i) (square-and-multiply over the log2 n bits of k i mod n) and by rho_t read as an integer from the per-cell
//      pass's array (one Keccak per cell there, none here), and writes the canonical term T_{t,i} = rho_t a_{t,i} -- the fold and LOCATE read them again.
// By count 2 log2 n + log2 l + 3 products per value.
struct KzgCoefArgs {
    const uint64_t* values;
    const uint32_t* cell; // labelled form
    const uint64_t* term_rho;
    uint64_t* term;
    const uint32_t* roots;
    uint64_t count;
    uint32_t log2n, log2l;
    Limbs9 omega_inv, into; // Montgomery-261
};
template <bool COSETS> __global__ void __launch_bounds__(CT) k_kzg_cell_coefficients(KzgCoefArgs P)
{
    __shared__ uint32_t s_w[COSETS ? 8 : 1][CT];
    const uint32_t tid = threadIdx.x, lgl = P.log2l, l = 1u << lgl, lgm = P.log2n - lgl, lgC = 8 - lgl, C = 1u << lgC;
    static_assert(CT == 256, "lgC = 8 - log2 l");
    const uint32_t g = tid >> lgl, j = tid & (l - 1u);
    const uint32_t i = lgl ? __brev(j) >> (32 - lgl) : 0u; // the coefficient this lane ends up with
    const FeT<FrP> into = fe_from<FrP>(P.into.d), omega_inv = fe_from<FrP>(P.omega_inv.d);
    for (uint64_t base = (uint64_t)blockIdx.x * C; base < P.count; base += (uint64_t)gridDim.x * C) {
        const uint64_t t = base + g;
        const bool live = t < P.count;
        uint32_t w[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, k = 0;
        if constexpr (COSETS) {
            const uint64_t t2 = base + (tid & (C - 1u));
            const uint32_t j2 = tid >> lgC;
            uint32_t w2[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            if (t2 < P.count) { // cell t2 = b m + k2: element b n + k2 + m j2 of the transforms
                const uint64_t b = t2 >> lgm, k2 = t2 & ((1ull << lgm) - 1ull);
                ld8(P.values + 4 * ((b << P.log2n) + k2 + ((uint64_t)j2 << lgm)), w2);
            }
            const uint32_t slot = ((tid & (C - 1u)) << lgl) + j2; // < C l = CT
#pragma unroll
            for (int q = 0; q < 8; q++) s_w[q][slot] = w2[q];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 8; q++) w[q] = s_w[q][tid];
            __syncthreads(); // the next trip writes the slots again
            k = (uint32_t)t & ((1u << lgm) - 1u);
        } else if (live) {
            ld8(P.values + 4 * ((t << lgl) + j), w);
            k = P.cell[t];
        }
        F2 x = mul(unpack<FrP>(w), into);
        uint32_t shift = 0; // the stage with half h takes the roots zeta^(-q l / (2 h)) = table[q << shift]
        for (uint32_t h = l >> 1; h; h >>= 1, shift++) {
            F2 p;
#pragma unroll
            for (int q = 0; q < NL; q++) p.d[q] = (uint32_t)__shfl_xor((int)x.d[q], (int)h);
            const bool upper = (j & h) != 0;
            const auto s = add(x, p);  // the lower lane's u + v
            const auto d = sub(p, x);  // the upper lane's u - v: u is the partner's
            Fe<FrP, 4, 5> y = d;
#pragma unroll
            for (int q = 0; q < NL; q++) y.d[q] = upper ? d.d[q] : s.d[q];
            const uint32_t* root = P.roots + NL * (upper ? (j & (h - 1u)) << shift : 0u); // entry 0 is one
            FeT<FrP> tw;
#pragma unroll
            for (int q = 0; q < NL; q++) tw.d[q] = root[q];
            x = mul(y, tw);
        }
        const uint32_t e = (k * i) & ((1u << P.log2n) - 1u); // k < 2^20, i < 64
        x = mul(x, pow_bits(omega_inv, e, (int)P.log2n));
        uint32_t rw[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, o[8];
        if (live) ld8(P.term_rho + 4 * t, rw);
        to_canonical(mul(x, unpack<FrP>(rw)), o);
        if (live) st8(P.term + 4 * ((t << lgl) + i), o, false);
    }
}

// ---- k_kzg_cells_fold: the sums over the cells t < cells, one workgroup per (range of cells, slot) ---------------------------------------------------------
// Slot k < S: sum of rho_t over the cells labelled k (which[t], or t >> log2 m in the open-cosets form); slot S + i: sum of T_{t,i}, written NEGATED (it is
// the scalar on P_i; zero stays zero).  Canonical additions modulo r (fr_sum_device.hpp) in a fixed tree, as k_kzg_fold: exact, so ranges and tree give the
// value any other order would.  With one range the workgroup writes the scalar itself; with more it writes a partial sum and k_kzg_cells_fold_finish
// adds the ranges up the same way.
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
// thread 0: the scalar of slot k from the sum -- on P_i the negated sum, on a commitment at infinity (a stand-in row) zero
__device__ __forceinline__ void put_slot(const uint64_t (&s)[4], uint32_t k, uint32_t S, unsigned long long skip_mask, uint64_t* __restrict__ out)
{
    uint64_t v[4] = { s[0], s[1], s[2], s[3] };
    if (k >= S && (v[0] | v[1] | v[2] | v[3]) != 0) { // r - sum: canonical, since 0 < sum < r
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
struct KzgCellsFoldArgs {
    const uint64_t *term_rho, *term;
    const uint32_t* which; // null: the label is t >> log2m
    uint32_t log2m, log2l, S;
    uint32_t cells, chunk; // range p is the cells [p chunk, min(cells, (p + 1) chunk))
    unsigned long long skip_mask;
    uint64_t* partial;     // [slot][range] x 4 words (more than one range)
    uint64_t* out;         // the first S + l scalars of A
};
__global__ void __launch_bounds__(CT) k_kzg_cells_fold(KzgCellsFoldArgs P)
{
    __shared__ uint64_t s_acc[CT][4];
    const uint32_t p = blockIdx.x, k = blockIdx.y;
    const uint32_t lo = p * P.chunk, hi = min(P.cells, lo + P.chunk); // lo < cells <= 2^20: no overflow
    uint64_t acc[4] = { 0, 0, 0, 0 };
    for (uint32_t t = lo + threadIdx.x; t < hi; t += CT) {
        uint64_t v[4];
        if (k < P.S) {
            const uint32_t label = P.which ? P.which[t] : t >> P.log2m;
            if (label != k) continue;
            ld4(P.term_rho + 4 * (size_t)t, v);
        } else {
            ld4(P.term + 4 * (((size_t)t << P.log2l) + (k - P.S)), v);
        }
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
__global__ void __launch_bounds__(CT) k_kzg_cells_fold_finish(const uint64_t* __restrict__ partial, uint32_t ranges, uint32_t S, unsigned long long skip_mask,
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

// ---- the layout entries (bbgpu_kzg_check_cells_layout, bbgpu_kzg_check_open_cosets_layout): up to 2^16 commitments ---------------------------------------
// The slot logic above costs O(S x cells) loads and (S + l) x 256 partial sums; these kernels replace its S commitment slots and leave the l slots of
// P_0 .. P_(l-1) to k_kzg_cells_fold (called with S = 0).  Resource usage of the gfx950 build (-Rpass-analysis=kernel-resource-usage), no scratch, no LDS
// but the scan's 2 KiB: k_kzg_layout_commitments 55 VGPRs, k_kzg_layout_hist 7, k_kzg_layout_scan 16, k_kzg_layout_scatter 13, k_kzg_layout_pieces 28,
// k_kzg_layout_finish 34.

// ONE COMMITMENT PER THREAD: what k_kzg_cells does to a proof -- the curve test, the resident row (the generator for infinity) -- on the raw words the
// caller handed over.  A wave writes the 64 infinity flags of its commitments as one word of the skip array (no atomics: the word is the wave's own); a
// wave that saw a finite point off the curve issues the two atomics of the findings, an honest call none.  Key of a finding: the commitment's index.  The
// thread also clears its label's counter for the histogram (labelled form).
struct KzgLayoutCommitArgs {
    const uint64_t* commitments;
    uint32_t* rows;
    uint64_t* skip;
    uint32_t* cnt; // null in the open-cosets form
    KzgFindings* find;
    uint32_t S;
};
__global__ void __launch_bounds__(CT) k_kzg_layout_commitments(KzgLayoutCommitArgs P)
{
    const uint32_t c = blockIdx.x * CT + threadIdx.x;
    uint32_t gen[16];
    store_affine_m261(gen, fe_from<Fq>(Fq::GEN_X), fe_from<Fq>(Fq::GEN_Y));
    bool off = false, inf = false;
    if (c < P.S) {
        inf = point_to_row(P.commitments + 8 * (size_t)c, gen, P.rows + (size_t)c * 16, &off);
        if (P.cnt) P.cnt[c] = 0;
    }
    const unsigned long long infs = __ballot(inf), offs = __ballot(off);
    if ((threadIdx.x & 63) != 0 || c >= P.S) return; // c is the wave's first commitment
    P.skip[c >> 6] = infs;
    if (!offs) return;
    atomicAdd(&P.find->bad_points, (unsigned long long)__popcll(offs));
    atomicMin(&P.find->first_key, (unsigned long long)c + (unsigned long long)(__ffsll((long long)offs) - 1));
}

// The cells grouped by label ONCE per call, a counting sort: the histogram (integer atomics on the S counters -- the order inside a list cannot change
// an exact sum), ONE workgroup's scan over the S <= 2^16 counters, the scatter into a permutation.  The scan writes two exclusive prefix sums: off[c], where
// the list of label c starts in the permutation, and poff[c], its first piece -- a list is cut into ceil(length / KZG_LAYOUT_PIECE) pieces -- and clears the
// counters again for the scatter, which counts them back up.
// The lanes of a wave that hold the same label meet first, so that a counter takes ONE atomic per wave that holds its label, not one per cell (2^14 cells
// on one label: 256 atomics on that counter; one per cell cost 0.19 ms in each of the two kernels, profiles/kzg_check_layout.txt): every lane, live or
// not, learns the lowest live lane with its label (its leader), its rank among those lanes and their number.  One trip per distinct label of the wave, at
// most 64, of ballots and compares on wave-uniform values; no memory access.
__device__ __forceinline__ void wave_groups(uint32_t label, bool live, uint32_t& leader, uint32_t& rank, uint32_t& size)
{
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(live);
    leader = lane;
    rank = 0;
    size = 1;
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const uint32_t lab = (uint32_t)__shfl((int)label, first);
        const bool mine = live && label == lab;
        const unsigned long long same = __ballot(mine); // holds lane `first`
        if (mine) {
            leader = (uint32_t)first;
            rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            size = (uint32_t)__popcll(same);
        }
        todo &= ~same;
    }
}
__global__ void __launch_bounds__(CT) k_kzg_layout_hist(const uint32_t* __restrict__ which, uint32_t count, uint32_t* __restrict__ cnt)
{
    const uint32_t t = blockIdx.x * CT + threadIdx.x;
    const bool live = t < count;
    const uint32_t c = live ? which[t] : 0u;
    uint32_t leader, rank, size;
    wave_groups(c, live, leader, rank, size);
    if (live && leader == (threadIdx.x & 63)) atomicAdd(&cnt[c], size);
}
// thread i takes the counters [i per, (i + 1) per), per = ceil(S / 256) <= 256: a sum, a scan of the 256 sums in LDS (every thread reaches every barrier),
// then the prefix sums of its own counters
__global__ void __launch_bounds__(CT) k_kzg_layout_scan(uint32_t* __restrict__ cnt, uint32_t S, uint32_t* __restrict__ off, uint32_t* __restrict__ poff)
{
    __shared__ uint32_t s_cells[CT], s_pieces[CT];
    const uint32_t per = (S + CT - 1) / CT, lo = min(S, threadIdx.x * per), hi = min(S, lo + per);
    uint32_t cells = 0, pieces = 0;
    for (uint32_t c = lo; c < hi; c++) {
        const uint32_t v = cnt[c];
        cells += v;
        pieces += (v + (uint32_t)KZG_LAYOUT_PIECE - 1u) / (uint32_t)KZG_LAYOUT_PIECE;
    }
    s_cells[threadIdx.x] = cells;
    s_pieces[threadIdx.x] = pieces;
    __syncthreads();
    for (uint32_t o = 1; o < CT; o <<= 1) { // inclusive scan
        const uint32_t a = threadIdx.x >= o ? s_cells[threadIdx.x - o] : 0u, b = threadIdx.x >= o ? s_pieces[threadIdx.x - o] : 0u;
        __syncthreads();
        s_cells[threadIdx.x] += a;
        s_pieces[threadIdx.x] += b;
        __syncthreads();
    }
    cells = s_cells[threadIdx.x] - cells;
    pieces = s_pieces[threadIdx.x] - pieces;
    for (uint32_t c = lo; c < hi; c++) {
        const uint32_t v = cnt[c];
        off[c] = cells;
        poff[c] = pieces;
        cnt[c] = 0;
        cells += v;
        pieces += (v + (uint32_t)KZG_LAYOUT_PIECE - 1u) / (uint32_t)KZG_LAYOUT_PIECE;
    }
    if (threadIdx.x == CT - 1) { // hi == S here
        off[S] = cells;
        poff[S] = pieces;
    }
}
__global__ void __launch_bounds__(CT) k_kzg_layout_scatter(const uint32_t* __restrict__ which, uint32_t count, const uint32_t* __restrict__ off,
                                                           uint32_t* __restrict__ cnt, uint32_t* __restrict__ perm)
{
    const uint32_t t = blockIdx.x * CT + threadIdx.x;
    const bool live = t < count;
    const uint32_t c = live ? which[t] : 0u;
    uint32_t leader, rank, size, base = 0;
    wave_groups(c, live, leader, rank, size);
    if (live && leader == (threadIdx.x & 63)) base = atomicAdd(&cnt[c], size);
    base = (uint32_t)__shfl((int)base, (int)leader); // every lane takes part; a lane past the end is its own leader
    if (live) perm[off[c] + base + rank] = t;
}

// the sum over a wave, left on every lane: the partner's words by __shfl_xor, canonical additions
__device__ __forceinline__ void wave_sum(uint64_t (&acc)[4])
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        uint64_t b[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)acc[i], o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(acc[i] >> 32), o);
            b[i] = ((uint64_t)hi << 32) | lo;
        }
        fr_add_canonical(acc, b);
    }
}
// ONE WAVE PER PIECE: the sum of rho_t over the at most KZG_LAYOUT_PIECE cells of one piece of one label's list that lie in the prefix t < cells (the test
// LOCATE's rounds need; the grouping is the call's).  At most KZG_LAYOUT_PIECE / 64 = 16 dependent additions per lane and the six of wave_sum, WHATEVER the
// labels are: a list of 2^20 / l cells is many pieces, not a long chain.  Labelled form: piece w belongs to the last label c with poff[c] <= w, found by a
// bisection of ceil(log2 S) wave-uniform steps.  Open-cosets form (perm null): label c is the cells [c m, (c + 1) m), each ceil(m / KZG_LAYOUT_PIECE) = pp
// pieces.  No barrier: a wave past the last piece leaves.
struct KzgLayoutFoldArgs {
    const uint64_t* term_rho;
    const uint32_t *perm, *off, *poff; // null in the open-cosets form
    const uint64_t* skip;
    uint32_t S, log2m, pp, cells;
    uint64_t* partial; // one sum per piece
    uint64_t* out;     // the S scalars on the commitments
};
__global__ void __launch_bounds__(CT) k_kzg_layout_pieces(KzgLayoutFoldArgs P)
{
    const uint32_t w = blockIdx.x * (CT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    uint32_t lo, hi;
    if (P.perm) {
        if (w >= P.poff[P.S]) return;
        uint32_t c = 0, e = P.S;
        while (e - c > 1) {
            const uint32_t mid = (c + e) >> 1;
            if (P.poff[mid] <= w) c = mid;
            else e = mid;
        }
        lo = P.off[c] + (w - P.poff[c]) * (uint32_t)KZG_LAYOUT_PIECE;
        hi = min(P.off[c + 1], lo + (uint32_t)KZG_LAYOUT_PIECE);
    } else {
        const uint32_t c = w / P.pp;
        if (c >= P.S) return;
        lo = (c << P.log2m) + (w - c * P.pp) * (uint32_t)KZG_LAYOUT_PIECE;
        hi = min((c + 1) << P.log2m, lo + (uint32_t)KZG_LAYOUT_PIECE);
    }
    uint64_t acc[4] = { 0, 0, 0, 0 };
    for (uint32_t i = lo + lane; i < hi; i += 64) {
        const uint32_t t = P.perm ? P.perm[i] : i;
        uint64_t v[4] = { 0, 0, 0, 0 };
        if (t < P.cells) ld4(P.term_rho + 4 * (size_t)t, v);
        fr_add_canonical(acc, v);
    }
    wave_sum(acc);
    if (lane != 0) return;
    ulonglong2* o2 = reinterpret_cast<ulonglong2*>(P.partial + 4 * (size_t)w);
    o2[0] = make_ulonglong2(acc[0], acc[1]);
    o2[1] = make_ulonglong2(acc[2], acc[3]);
}
// ONE WAVE PER LABEL over the sums of its pieces (at most 2^20 / KZG_LAYOUT_PIECE = 1024 of them: 16 additions per lane); a label that owns no cell and
// a commitment at infinity (its bit in the skip array: the row is a stand-in) get the scalar zero
__global__ void __launch_bounds__(CT) k_kzg_layout_finish(KzgLayoutFoldArgs P)
{
    const uint32_t c = blockIdx.x * (CT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= P.S) return;
    const uint32_t lo = P.perm ? P.poff[c] : c * P.pp, hi = P.perm ? P.poff[c + 1] : lo + P.pp;
    uint64_t acc[4] = { 0, 0, 0, 0 };
    for (uint32_t p = lo + lane; p < hi; p += 64) {
        uint64_t v[4];
        ld4(P.partial + 4 * (size_t)p, v);
        fr_add_canonical(acc, v);
    }
    wave_sum(acc);
    if (lane != 0) return;
    const bool skip = ((P.skip[c >> 6] >> (c & 63u)) & 1ull) != 0;
    ulonglong2* o2 = reinterpret_cast<ulonglong2*>(P.out + 4 * (size_t)c);
    o2[0] = make_ulonglong2(skip ? 0 : acc[0], skip ? 0 : acc[1]);
    o2[1] = make_ulonglong2(skip ? 0 : acc[2], skip ? 0 : acc[3]);
}

} // namespace

// the most pieces the lists of `count` cells under S labels can have (sum of ceil(n_c / PIECE) <= count / PIECE + the labels that own a cell)
size_t kzg_layout_max_pieces(size_t count, size_t S, int log2m, bool cosets)
{
    if (cosets) return S * ((((size_t)1 << log2m) + KZG_LAYOUT_PIECE - 1) / KZG_LAYOUT_PIECE);
    return count / KZG_LAYOUT_PIECE + std::min(count, S);
}

// The commitments tested and written as rows, their skip bits and findings (L.find: a KzgFindings the caller has initialised, {0, ~0}); in the labelled
// form (L.which given) also the grouping of the cells by label.  Once per call.  ms: the device time of these kernels from events, with one synchronisation
int kzg_layout_group(const KzgLayoutBuffers& L, size_t count, size_t S, hipStream_t st, float* ms)
{
    StageEvents<2> ev;
    if (int rc = ev.create(ms != nullptr)) return rc;
    if (int rc = ev.mark(0, st)) return rc;
    KzgLayoutCommitArgs P{};
    P.commitments = L.commitments;
    P.rows = L.rows;
    P.skip = L.skip;
    P.cnt = L.which ? L.cnt : nullptr;
    P.find = L.find;
    P.S = (uint32_t)S;
    k_kzg_layout_commitments<<<blocks_of((uint32_t)S, CT), CT, 0, st>>>(P);
    if (L.which) {
        k_kzg_layout_hist<<<blocks_of((uint32_t)count, CT), CT, 0, st>>>(L.which, (uint32_t)count, L.cnt);
        k_kzg_layout_scan<<<1, CT, 0, st>>>(L.cnt, (uint32_t)S, L.off, L.poff);
        k_kzg_layout_scatter<<<blocks_of((uint32_t)count, CT), CT, 0, st>>>(L.which, (uint32_t)count, L.off, L.cnt, L.perm);
    }
    HIPCHK(launch_check());
    if (ms) {
        if (int rc = ev.mark(1, st)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = ev.ms(0, 1, ms)) return rc;
    }
    return BBGPU_OK;
}

// the scalars on the S commitments over the cells [0, cells) of a call of `count` cells, after kzg_layout_group on the same stream: d_out[c], c < S
int kzg_layout_fold(const KzgLayoutBuffers& L, const uint64_t* d_term_rho, size_t cells, size_t count, size_t S, int log2m, uint64_t* d_out, hipStream_t st,
                    float* ms)
{
    StageEvents<2> ev;
    if (int rc = ev.create(ms != nullptr)) return rc;
    if (int rc = ev.mark(0, st)) return rc;
    KzgLayoutFoldArgs P{};
    P.term_rho = d_term_rho;
    P.perm = L.which ? L.perm : nullptr;
    P.off = L.which ? L.off : nullptr;
    P.poff = L.which ? L.poff : nullptr;
    P.skip = L.skip;
    P.S = (uint32_t)S;
    P.log2m = (uint32_t)log2m;
    P.pp = (uint32_t)((((size_t)1 << log2m) + KZG_LAYOUT_PIECE - 1) / KZG_LAYOUT_PIECE);
    P.cells = (uint32_t)cells;
    P.partial = L.partial;
    P.out = d_out;
    const uint32_t pieces = (uint32_t)kzg_layout_max_pieces(count, S, log2m, L.which == nullptr);
    k_kzg_layout_pieces<<<blocks_of(pieces, CT / 64), CT, 0, st>>>(P);
    k_kzg_layout_finish<<<blocks_of((uint32_t)S, CT / 64), CT, 0, st>>>(P);
    HIPCHK(launch_check());
    if (ms) {
        if (int rc = ev.mark(1, st)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = ev.ms(0, 1, ms)) return rc;
    }
    return BBGPU_OK;
}

// B.find: one KzgFindings the caller has initialised ({0, ~0})
int kzg_cells_claims(const KzgCellsBuffers& B, const uint64_t seed[4], size_t count, int log2n, int log2l, const uint32_t psi_m261[9], hipStream_t st)
{
    KzgCellsArgs P{};
    P.proofs = B.proofs;
    P.cell = B.cell;
    P.rows = B.rows;
    P.scal_a = B.scal_a;
    P.scal_b = B.scal_b;
    P.term_rho = B.term_rho;
    P.find = B.find;
    P.count = count;
    P.log2m = (uint32_t)(log2n - log2l);
    P.psi = to_limbs9(psi_m261);
    for (int k = 0; k < 4; k++) P.seed.d[k] = seed[k];
    k_kzg_cells<<<kzg_check_claim_threads(count) / CT, CT, 0, st>>>(P);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// after kzg_cells_claims on the same stream (it reads rho_t); ms: the device time of the kernel from events, with one synchronisation
int kzg_cells_coefficients(const KzgCellsBuffers& B, size_t count, int log2n, int log2l, const uint32_t omega_inv_m261[9], const uint32_t into_m261[9],
                           hipStream_t st, float* ms)
{
    StageEvents<2> ev;
    if (int rc = ev.create(ms != nullptr)) return rc;
    KzgCoefArgs P{};
    P.values = B.values;
    P.cell = B.cell;
    P.term_rho = B.term_rho;
    P.term = B.term;
    P.roots = B.roots;
    P.count = count;
    P.log2n = (uint32_t)log2n;
    P.log2l = (uint32_t)log2l;
    P.omega_inv = to_limbs9(omega_inv_m261);
    P.into = to_limbs9(into_m261);
    const size_t per = (size_t)CT >> log2l; // cells per workgroup
    const uint32_t blocks = (uint32_t)std::min<size_t>((count + per - 1) / per, KZG_CELLS_COEF_MAX_BLOCKS);
    if (int rc = ev.mark(0, st)) return rc;
    if (B.cell) k_kzg_cell_coefficients<false><<<blocks, CT, 0, st>>>(P);
    else k_kzg_cell_coefficients<true><<<blocks, CT, 0, st>>>(P);
    HIPCHK(launch_check());
    if (ms) {
        if (int rc = ev.mark(1, st)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = ev.ms(0, 1, ms)) return rc;
    }
    return BBGPU_OK;
}

int kzg_cells_fold(const KzgCellsBuffers& B, size_t cells, size_t S, int log2n, int log2l, uint64_t skip_mask, uint64_t* d_out, hipStream_t st)
{
    KzgCellsFoldArgs P{};
    P.term_rho = B.term_rho;
    P.term = B.term;
    P.which = B.which;
    P.log2m = (uint32_t)(log2n - log2l);
    P.log2l = (uint32_t)log2l;
    P.S = (uint32_t)S;
    P.cells = (uint32_t)cells;
    const uint32_t ranges = kzg_check_fold_ranges(cells), slots = (uint32_t)(S + ((size_t)1 << log2l));
    P.chunk = (uint32_t)(((cells + ranges - 1) / ranges + CT - 1) / CT * CT);
    P.skip_mask = skip_mask;
    P.partial = B.partial;
    P.out = d_out;
    k_kzg_cells_fold<<<dim3(ranges, slots), CT, 0, st>>>(P);
    if (ranges > 1) k_kzg_cells_fold_finish<<<slots, CT, 0, st>>>(B.partial, ranges, (uint32_t)S, skip_mask, d_out);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
