// poly.hip -- device-resident polynomial helpers over Fr for gfx950: the scan-shaped and pointwise O(n) pieces of the
// PLONK prover that sit between the NTTs and the MSMs.
//
// Replaces, on resident vectors, the reference's serial / OpenMP-chunked CPU loops
//   polynomial_arithmetic::evaluate                              polynomials/polynomial_arithmetic.cpp:337-373
//   polynomial_arithmetic::compute_kate_opening_coefficients     :562-591
//   polynomial_arithmetic::compute_lagrange_polynomial_fft       :381-476
//   polynomial_arithmetic::divide_by_pseudo_vanishing_polynomial :478-560
//   fr::batch_invert                                             fields/field.hpp:503-522
//   the grand-product prefix products                            waffle/proof_system/prover/prover.cpp:194-202
//   compute_permutation_lagrange_base_single                     waffle/proof_system/permutation.hpp:15-87
// adds what the reference has no counterpart of: evaluation and opening of polynomials given by their VALUES on the domain (the k_bary_* kernels and
// bary_open: barycentric sums over one shared batch inversion, no transform; bary_inverses / bary_open_with / bary_open_folded: the same at several
// points of an opening session over ONE inversion, and the opening of a fold of polynomials -- k_bary_fold_dot, k_fold),
// and provides the fused pointwise kernels of the prover rounds (prover.cpp:135-222,224-300,302-403,461-463,520-528,567-595,
// arithmetic_widget.cpp:66-104,106-126).
//
// Data format: every vector is the reference's own (n x 4 x u64, Montgomery 2^256), read as any representative below 2^256
// and always written canonical.  Kernel constants arrive as canonical 9 x 29-bit limbs in one of two forms (host_fr.hpp):
//   *_m256 : x * 2^256, the memory form -- adds to / subtracts from loaded values;
//   *_m261 : x * 2^261 -- a multiplier: mont261(a * 2^256, x * 2^261) = a x * 2^256 stays in memory form.
// A raw product of k memory-form values carries 2^(261 - 5k); one multiplication by FIXk = 2^(256 + 5k) repairs it.
// Sequences like g * w^i are generated in-kernel in the 2^261 form: thread t raises the base to t from a table of
// base^(2^j) and then strides by base^T, so no root table is read from memory.
//
// Scans: the serial chains of the reference (prefix products, Horner suffix sums) become three-phase workgroup scans:
// per-thread runs of 8 elements, a Hillis-Steele doubling over the 256 thread partials in LDS, a single-workgroup scan
// of the block partials, and a final pass that applies the carries.  Exact field arithmetic makes the result independent
// of the association order, so outputs are bit-identical to the serial loops.
//
// One text per kernel: a scan phase, an evaluation or a pointwise operation that serves both the single-vector helpers of
// the C ABI and the lanes of the prover is ONE device body, wrapped twice -- k_x(Args by value) and k_x_tab / k_x_lanes
// (const Args* table, blockIdx.y = record) -- and one host driver issues either (scan_issue, below).  The bodies take
// U = true only where their constants are fields of a table record (see cst).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "bbgpu_internal.h"
#include "fe.hpp"
#include "host_fr.hpp"
#include "host_lagrange_open.hpp"
#include "poly.h"

namespace bbgpu {
namespace poly {

using Fr = FrP;
using FrC = FeT<Fr>;      // canonical constant
using FrV = Fe<Fr, 1, 6>; // a loaded memory value (< 2^256 < 6r)
using FrM = Fe<Fr, 1, 2>; // a fresh product

constexpr int PT = 256;  // threads per workgroup of the pointwise kernels
constexpr int RUN = 8;   // elements per thread in the scan kernels
constexpr int SCAN_T = 256;
constexpr int SCAN_BLOCK = SCAN_T * RUN; // 2048 elements per workgroup

// ---- device helpers -------------------------------------------------------------------------------------------------
__device__ __forceinline__ FrV ldv(const uint32_t* __restrict__ p, size_t i)
{
    const uint4* q = reinterpret_cast<const uint4*>(p + i * 8);
    const uint4 a = q[0], b = q[1];
    const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
    return unpack<Fr>(w);
}
template <int L, int V> __device__ __forceinline__ void stv(uint32_t* __restrict__ p, size_t i, const Fe<Fr, L, V>& v)
{
    uint32_t w[8];
    to_canonical(v, w);
    uint4* q = reinterpret_cast<uint4*>(p + i * 8);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
// U: the constant is a field of a record in a device table (the lane-batched kernels below), written by the host before the launch and by nobody
// during it, and every lane of the workgroup reads the same record: it is read as constant memory, i.e. through the scalar cache into scalar
// registers, where a by-value kernel argument would have been.  Only for fields of such records: never for a local.
template <bool U = false> __device__ __forceinline__ FrC cst(const Limbs9& c)
{
    if (!U) return fe_from<Fr>(c.d);
    FrC r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.d[i] = ((const __attribute__((address_space(4))) uint32_t*)c.d)[i];
    return r;
}
__device__ __forceinline__ FrC fix2() { return fe_from<Fr>(Fr::M256_TO_M261); }
__device__ __forceinline__ FrC fix3() { return fe_from<Fr>(Fr::FIX3); }
__device__ __forceinline__ FrC fix4() { return fe_from<Fr>(Fr::FIX4); }
// value * value -> memory form
template <int L1, int V1, int L2, int V2> __device__ __forceinline__ FrM mulv(const Fe<Fr, L1, V1>& a, const Fe<Fr, L2, V2>& b)
{
    return mul(mul(a, b), fix2());
}
template <class F, int L, int V> __device__ __forceinline__ Fe<F, 1, 2> tight2(const Fe<F, L, V>& a)
{
    // squeeze a lazy value back to the (1, 2) loop-carried type with one multiplication by one (2^261 form)
    return mul(a, fe_from<F>(F::ONE));
}
using FrH = Fe<Fr, 2, 8>; // loop-carried Horner accumulator: (product) + (loaded value), fed straight into the next multiply

// start * base^e, start in either form (the result keeps it); T.p[j] = base^(2^j) in the 2^261 form
template <bool U = false> __device__ __forceinline__ FrM pow_tab(const PowTab& T, uint32_t e, const Limbs9& start)
{
    FrM acc = mul(cst(start), fe_from<Fr>(Fr::ONE)); // (plain read: `start` may be a local of the caller, not a table field)
    for (int j = 0; e; j++, e >>= 1)
        if (e & 1) acc = mul(acc, cst<U>(T.p[j]));
    return acc;
}

// ---- small utility kernels ------------------------------------------------------------------------------------------
// out[i] = start * base^i  (start_m256 -> a table in memory form)
__global__ void __launch_bounds__(PT) k_powers(uint32_t* __restrict__ out, uint32_t n, PowTab T, Limbs9 start_m256, Limbs9 step_m261)
{
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    FrM x = pow_tab(T, t, start_m256);
    const FrC step = cst(step_m261);
    for (uint32_t i = t; i < n; i += nt) {
        stv(out, i, x);
        x = mul(x, step);
    }
}
// dst[0..n_dst) = src[0..n_src) followed by zeros (polynomial(other, size): polynomial.cpp:48-66), bit for bit; with an optional per-record multiplier:
// alpha Z and beta sigma_i are scaled in coefficient form, in front of the lanes' shared plain transform (the *_WITH_CONSTANT kinds take one constant
// per batched launch; scaling commutes with the transform and every value is exact)
template <bool U> __device__ __forceinline__ void copy_pad_body(const CopyPadArgs& A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_dst) return;
    uint4* q = reinterpret_cast<uint4*>(A.dst + (size_t)i * 8);
    if (i >= A.n_src) {
        q[0] = make_uint4(0, 0, 0, 0);
        q[1] = make_uint4(0, 0, 0, 0);
    } else if (A.scaled) {
        stv(A.dst, i, mul(ldv(A.src, i), cst<U>(A.c_m261)));
    } else {
        const uint4* sp = reinterpret_cast<const uint4*>(A.src + (size_t)i * 8);
        q[0] = sp[0];
        q[1] = sp[1];
    }
}
__global__ void __launch_bounds__(PT) k_copy_pad(CopyPadArgs A) { copy_pad_body<false>(A); }
__global__ void __launch_bounds__(PT) k_copy_pad_lanes(const CopyPadArgs* __restrict__ tab) { copy_pad_body<true>(tab[blockIdx.y]); }
// out[i] = a[i] * b[i] * c   (c in the 2^261 form, already carrying the FIX2 factor: c' = c * 2^5)
template <bool U> __device__ __forceinline__ void mul2c_body(const Mul2cArgs& A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    stv(A.out, i, mul(mul(ldv(A.a, i), ldv(A.b, i)), cst<U>(A.c_fix_m261)));
}
__global__ void __launch_bounds__(PT) k_mul2c(Mul2cArgs A) { mul2c_body<false>(A); }
__global__ void __launch_bounds__(PT) k_mul2c_lanes(const Mul2cArgs* __restrict__ tab) { mul2c_body<true>(tab[blockIdx.y]); }
// out[i] = a[i] * b[i]     (polynomial_arithmetic::mul, :328-335)
__global__ void __launch_bounds__(PT) k_mul(uint32_t* __restrict__ out, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    stv(out, i, mulv(ldv(a, i), ldv(b, i)));
}

// ---- scans ----------------------------------------------------------------------------------------------------------
// MODE 0: running product  y_i = prod of x over the scanned prefix        (identity 1, combine a * b)
// MODE 1: Horner sums      y_i = sum_{j >= i} x_j z^(j - i)               (suffix; combine y_i = x_i + z^len(i..) * y_next)
// Both are scans of an associative operation; DIR selects prefix (0) or suffix (1) for MODE 0, MODE 1 is always suffix.
// Values travel between phases in memory form (canonical), so the three phases compose exactly.
struct ScanArgs {
    const uint32_t* in;   // n elements
    uint32_t* out;        // n elements (phase 3)
    uint32_t* tpart;      // per-thread partial, exclusive within its block: ceil(n / RUN) elements
    uint32_t* bpart;      // per-block total: ceil(n / SCAN_BLOCK) elements
    const uint32_t* bcarry; // per-block exclusive carry (phase 3)
    uint32_t n;
    uint32_t reverse;     // MODE 0: 1 = suffix products
    uint32_t inclusive;   // output includes element i itself
    uint32_t has_carry;   // 0: top level, bcarry is not read
    uint32_t fused_nb;    // phase 3, <= SCAN_T blocks: every workgroup scans the bpart[0..fused_nb) block totals itself instead of reading bcarry
    uint32_t* total_out;  // fused: where block 0 leaves the combination of everything
    Limbs9 zpow[20];      // MODE 1: z^(RUN * 2^j), j < 8, for the thread-level doubling (2^261 form); [8] = z, [9] = z^RUN;
                          // [12 + j] = z^(SCAN_BLOCK * 2^j), j < 8: the doubling over whole blocks of the fused phase 3
};

// LDS doubling scan over the SCAN_T thread partials of a block.  v = this thread's inclusive partial on entry; returns the
// exclusive partial (combination of all LATER threads for suffix scans / EARLIER threads for prefix scans).
template <int MODE, int ZB = 0, bool U = false> __device__ __forceinline__ FrM block_scan(FrM v, uint32_t* sh, bool towards_high, const ScanArgs& A, FrM* total)
{
    // position p runs in scan order: p = 0 is the first element combined
    const uint32_t t = threadIdx.x;
    const uint32_t p = towards_high ? t : (SCAN_T - 1 - t);
    // inclusive Hillis-Steele over positions: after step j, v_p = combine(v_{p - 2^j .. p})
    uint32_t* buf = sh;
#pragma unroll 1
    for (int j = 0, off = 1; off < SCAN_T; j++, off <<= 1) {
#pragma unroll
        for (int k = 0; k < NL; k++) buf[k * SCAN_T + p] = v.d[k];
        __syncthreads();
        if (p >= (uint32_t)off) {
            FrM o;
#pragma unroll
            for (int k = 0; k < NL; k++) o.d[k] = buf[k * SCAN_T + p - off];
            if (MODE == 0) {
                v = mulv(v, o);
            } else {
                // suffix Horner: scan order runs from the highest index down; position p holds S over `off` earlier
                // positions: S_new = S_here + z^(RUN * off) * S_earlier ... earlier positions are HIGHER indices, so
                // S(i..) = S_here + z^(len_here) * S_later with len_here = RUN * off thread-runs combined so far
                v = tight2<Fr>(add(v, mul(o, cst<U>(A.zpow[ZB + j]))));
            }
        }
        __syncthreads();
    }
    // v is now inclusive over positions 0..p; the exclusive value is position p-1's inclusive value
#pragma unroll
    for (int k = 0; k < NL; k++) buf[k * SCAN_T + p] = v.d[k];
    __syncthreads();
    FrM ex;
    if (p == 0) {
        if (MODE == 0) ex = mul(fe_from<Fr>(Fr::ONE_M256), fe_from<Fr>(Fr::ONE)); // memory-form one
        else ex = mul(fe_zero<Fr>(), fe_from<Fr>(Fr::ONE));
    } else {
#pragma unroll
        for (int k = 0; k < NL; k++) ex.d[k] = buf[k * SCAN_T + p - 1];
    }
    FrM tot;
#pragma unroll
    for (int k = 0; k < NL; k++) tot.d[k] = buf[k * SCAN_T + SCAN_T - 1];
    *total = tot;
    __syncthreads();
    return ex;
}

// identity-padded load: MODE 0 pads with one, MODE 1 with zero
template <int MODE> __device__ __forceinline__ FrV ld_or_id(const uint32_t* p, uint32_t i, uint32_t n)
{
    if (i < n) return ldv(p, i);
    FrV r;
    if (MODE == 0) {
#pragma unroll
        for (int k = 0; k < NL; k++) r.d[k] = Fr::ONE_M256[k];
    } else {
#pragma unroll
        for (int k = 0; k < NL; k++) r.d[k] = 0;
    }
    return r;
}

// phase 1: per-thread run totals, block scan of them -> tpart (exclusive within the block), bpart (block total)
template <int MODE, bool U> __device__ __forceinline__ void scan_phase1_body(const ScanArgs& A, uint32_t* sh)
{
    if (blockIdx.x * SCAN_BLOCK >= A.n) return; // whole workgroup
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    const uint32_t base = b * SCAN_BLOCK + t * RUN;
    const bool suffix = (MODE == 1) || A.reverse;
    FrM run;
    if (MODE == 0) {
        FrV x0 = ld_or_id<0>(A.in, base, A.n);
        run = mul(x0, fe_from<Fr>(Fr::ONE)); // memory form kept
#pragma unroll
        for (int k = 1; k < RUN; k++) run = mulv(run, ld_or_id<0>(A.in, base + k, A.n));
    } else {
        // E = sum_k x_{base+k} z^k, Horner from the top
        const FrC z = cst<U>(A.zpow[8]);
        FrH h = ld_or_id<1>(A.in, base + RUN - 1, A.n);
#pragma unroll
        for (int k = RUN - 2; k >= 0; k--) h = add(mul(h, z), ld_or_id<1>(A.in, base + k, A.n));
        run = tight2<Fr>(h);
    }
    FrM total;
    FrM ex = block_scan<MODE, 0, U>(run, sh, !suffix, A, &total);
    const uint32_t tid = b * SCAN_T + t;
    if ((size_t)tid * RUN < A.n) stv(A.tpart, tid, ex);
    if (t == 0) stv(A.bpart, b, total);
}
// one scan, its arguments by value
template <int MODE> __global__ void __launch_bounds__(SCAN_T) k_scan_phase1(ScanArgs A)
{
    __shared__ uint32_t sh[NL * SCAN_T];
    scan_phase1_body<MODE, false>(A, sh);
}
// the same over a device table of jobs (blockIdx.y = job): the lanes of a proof batch, two scans each
template <int MODE> __global__ void __launch_bounds__(SCAN_T) k_scan_phase1_tab(const ScanArgs* __restrict__ tab)
{
    __shared__ uint32_t sh[NL * SCAN_T];
    scan_phase1_body<MODE, true>(tab[blockIdx.y], sh);
}

// phase 3: out_i from the block carry, the thread partial and the in-run elements
template <int MODE, bool U> __device__ __forceinline__ void scan_phase3_body(const ScanArgs& A, uint32_t* sh)
{
    const uint32_t t = threadIdx.x, b = blockIdx.x;
    if (b * SCAN_BLOCK >= A.n) return; // whole workgroup (n = 0: a job without an output vector, where the total does not come from this phase)
    const bool suffix = (MODE == 1) || A.reverse;
    // <= SCAN_T blocks: the exclusive scan of the block totals (phase 1 + phase 3 of the nested level: two launches of one workgroup
    // each, ~40 us of a 2^16-element scan's ~95) is done here by every workgroup for itself, lane t standing for block t
    FrM carry = mul(fe_zero<Fr>(), fe_from<Fr>(Fr::ONE));
    if (A.fused_nb) {
        FrM v;
        if (MODE == 0) {
            v = mul(ld_or_id<0>(A.bpart, t, A.fused_nb), fe_from<Fr>(Fr::ONE));
        } else {
            FrH h = ld_or_id<1>(A.bpart, t, A.fused_nb);
            v = tight2<Fr>(h);
        }
        FrM total;
        const FrM ex = block_scan<MODE, 12, U>(v, sh, !suffix, A, &total);
        if (t == b) {
#pragma unroll
            for (int k = 0; k < NL; k++) sh[k] = ex.d[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NL; k++) carry.d[k] = sh[k];
        if (b == 0 && t == 0 && A.total_out) stv(A.total_out, 0, total);
    }
    const uint32_t base = b * SCAN_BLOCK + t * RUN;
    if (base >= A.n || !A.out) return; // (a scan wanted for its total only has no output vector)
    const uint32_t tid = b * SCAN_T + t;
    if (MODE == 0) {
        FrM acc = mul(ldv(A.tpart, tid), fe_from<Fr>(Fr::ONE)); // everything before (after) this run
        if (A.fused_nb) acc = mulv(carry, ldv(A.tpart, tid));
        else if (A.has_carry) acc = mulv(ldv(A.bcarry, b), ldv(A.tpart, tid));
        if (!suffix) {
            for (uint32_t k = 0; k < RUN && base + k < A.n; k++) {
                const FrV x = ldv(A.in, base + k);
                if (A.inclusive) {
                    acc = mulv(acc, x);
                    stv(A.out, base + k, acc);
                } else {
                    stv(A.out, base + k, acc);
                    acc = mulv(acc, x);
                }
            }
        } else {
            for (int k = RUN - 1; k >= 0; k--) {
                if (base + k >= A.n) continue;
                const FrV x = ldv(A.in, base + k);
                if (A.inclusive) {
                    acc = mulv(acc, x);
                    stv(A.out, base + k, acc);
                } else {
                    stv(A.out, base + k, acc);
                    acc = mulv(acc, x);
                }
            }
        }
    } else {
        // carry into this run: S at index base + RUN = tpart + z^(RUN * (threads after t in the block)) * bcarry
        const uint32_t after = SCAN_T - 1 - t;
        FrM zp = mul(fe_from<Fr>(Fr::ONE), fe_from<Fr>(Fr::ONE)); // one in the 2^261 form
        for (int j = 0; j < 8; j++)
            if ((after >> j) & 1) zp = mul(zp, cst<U>(A.zpow[j]));
        FrH acc = ldv(A.tpart, tid);
        if (A.fused_nb) acc = add(mul(carry, zp), ldv(A.tpart, tid));
        else if (A.has_carry) acc = add(mul(ldv(A.bcarry, b), zp), ldv(A.tpart, tid));
        const FrC z = cst<U>(A.zpow[8]);
        for (int k = RUN - 1; k >= 0; k--) {
            if (base + k >= A.n) continue; // padded zeros do not change acc
            const FrV x = ldv(A.in, base + k);
            if (A.inclusive) {
                acc = add(mul(acc, z), x);
                stv(A.out, base + k, acc);
            } else {
                stv(A.out, base + k, acc);
                acc = add(mul(acc, z), x);
            }
        }
    }
}
template <int MODE> __global__ void __launch_bounds__(SCAN_T) k_scan_phase3(ScanArgs A)
{
    __shared__ uint32_t sh[NL * SCAN_T];
    scan_phase3_body<MODE, false>(A, sh);
}
template <int MODE> __global__ void __launch_bounds__(SCAN_T, MODE == 0 ? 7 : 8) k_scan_phase3_tab(const ScanArgs* __restrict__ tab)
{
    __shared__ uint32_t sh[NL * SCAN_T];
    scan_phase3_body<MODE, true>(tab[blockIdx.y], sh);
}

// ---- evaluate: sum_i c_i z^i ------------------------------------------------------------------------------------------
// dst[i] = the workgroup's sum of one value per thread, by a tree in LDS (lazy adds: 8 levels of doubling the bound stay far below the limits after a
// tighten per level)
__device__ __forceinline__ void block_sum(uint32_t* __restrict__ dst, size_t i, const FrM& acc, uint32_t* sh)
{
#pragma unroll
    for (int k = 0; k < NL; k++) sh[k * PT + threadIdx.x] = acc.d[k];
    __syncthreads();
    for (uint32_t half = PT / 2; half >= 1; half >>= 1) {
        if (threadIdx.x < half) {
            FrM a, b;
#pragma unroll
            for (int k = 0; k < NL; k++) {
                a.d[k] = sh[k * PT + threadIdx.x];
                b.d[k] = sh[k * PT + threadIdx.x + half];
            }
            FrM sm = tight2<Fr>(add(a, b));
#pragma unroll
            for (int k = 0; k < NL; k++) sh[k * PT + threadIdx.x] = sm.d[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        FrM sm;
#pragma unroll
        for (int k = 0; k < NL; k++) sm.d[k] = sh[k * PT];
        stv(dst, i, sm);
    }
}
// thread t owns indices t, t + T, t + 2T, ... (T = nblocks * PT threads): Horner in z^T from the top, then * z^t; one partial / block
template <bool U>
__device__ __forceinline__ void eval_partial_body(const uint32_t* __restrict__ c, uint32_t n, uint32_t nblocks, const PowTab& T, const Limbs9& zT_m261,
                                                  uint32_t* __restrict__ partial, uint32_t* sh)
{
    if (blockIdx.x >= nblocks) return; // (the jobs of a table share one grid: the widest job's)
    const uint32_t nt = nblocks * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    FrM acc = mul(fe_zero<Fr>(), fe_from<Fr>(Fr::ONE));
    if (t < n) {
        const uint32_t cnt = (n - t + nt - 1) / nt;
        const FrC zT = cst<U>(zT_m261);
        FrH h = ldv(c, t + (size_t)(cnt - 1) * nt);
        for (uint32_t k = cnt - 1; k-- > 0;) h = add(mul(h, zT), ldv(c, t + (size_t)k * nt));
        Limbs9 one261;
#pragma unroll
        for (int k = 0; k < NL; k++) one261.d[k] = Fr::ONE[k];
        acc = mul(h, pow_tab<U>(T, t, one261)); // * z^t
    }
    block_sum(partial, blockIdx.x, acc, sh);
}
__global__ void __launch_bounds__(PT) k_eval_partial(const uint32_t* __restrict__ c, uint32_t n, PowTab T, Limbs9 zT_m261, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t sh[NL * PT];
    eval_partial_body<false>(c, n, gridDim.x, T, zT_m261, partial, sh);
}
// any number of evaluations, each at a point of its own, from a device table of jobs (blockIdx.y = job): the openings of every lane of a proof batch
// (the prover's seven openings at z / z w, prover.cpp:478-512)
__global__ void __launch_bounds__(PT) k_eval_partial_tab(const EvalTabJob* __restrict__ tab)
{
    __shared__ uint32_t sh[NL * PT];
    const EvalTabJob& J = tab[blockIdx.y];
    eval_partial_body<true>(J.c, J.n, J.blocks, J.T, J.zT, J.partial, sh);
}
// result[0] = sum of `count` partials (count <= a few hundred): one workgroup
__device__ __forceinline__ void sum_small_body(const uint32_t* __restrict__ partial, uint32_t count, uint32_t* __restrict__ result, uint32_t* sh)
{
    FrM acc = mul(fe_zero<Fr>(), fe_from<Fr>(Fr::ONE));
    for (uint32_t i = threadIdx.x; i < count; i += PT) acc = tight2<Fr>(add(acc, ldv(partial, i)));
    block_sum(result, 0, acc, sh);
}
__global__ void __launch_bounds__(PT) k_sum_small(const uint32_t* __restrict__ partial, uint32_t count, uint32_t* __restrict__ out)
{
    __shared__ uint32_t sh[NL * PT];
    sum_small_body(partial, count, out, sh);
}
__global__ void __launch_bounds__(PT) k_sum_small_tab(const EvalTabJob* __restrict__ tab)
{
    __shared__ uint32_t sh[NL * PT];
    const EvalTabJob& J = tab[blockIdx.x];
    sum_small_body(J.partial, J.blocks, J.result, sh);
}

// ---- prover round kernels -------------------------------------------------------------------------------------------
// permutation.hpp:15-87: sigma[i] = k_type * w^(mapping & mask), gathered from the table of subgroup elements
__global__ void __launch_bounds__(PT) k_sigma_from_mapping(uint32_t* __restrict__ out, const uint32_t* __restrict__ mapping,
                                                         const uint32_t* __restrict__ roots, uint32_t n, Limbs9 k1_m261, Limbs9 k2_m261)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = mapping[i];
    const uint32_t idx = (m & ((1u << 29) - 1u)) & (n - 1);
    const FrV w = ldv(roots, idx);
    switch ((m >> 30) & 3u) {
    case 2: stv(out, i, mul(w, cst(k2_m261))); break;
    case 1: stv(out, i, mul(w, cst(k1_m261))); break;
    default: stv(out, i, w); break;
    }
}

// prover.cpp:148-187: numerator / denominator factors of the grand product, three wires multiplied together
//   num_i = (w_l + beta w^i + gamma)(w_r + beta k1 w^i + gamma)(w_o + beta k2 w^i + gamma)
//   den_i = (w_l + beta sigma_1 + gamma)(w_r + beta sigma_2 + gamma)(w_o + beta sigma_3 + gamma)
__device__ __forceinline__ void z_terms_body(const ZTermsArgs& A)
{
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n) return;
    Limbs9 one261;
#pragma unroll
    for (int k = 0; k < NL; k++) one261.d[k] = Fr::ONE[k];
    FrM x = pow_tab<true>(A.root, t, one261); // w^t, 2^261 form
    const FrC step = cst<true>(A.step_m261), beta = cst<true>(A.beta_m256), bk1 = cst<true>(A.beta_k1_m256), bk2 = cst<true>(A.beta_k2_m256), gamma = cst<true>(A.gamma_m256),
              beta261 = cst<true>(A.beta_m261);
    for (uint32_t i = t; i < A.n; i += nt) {
        const FrV wl = ldv(A.w_l, i), wr = ldv(A.w_r, i), wo = ldv(A.w_o, i);
        auto a0 = add(add(mul(x, beta), gamma), wl);
        auto a1 = add(add(mul(x, bk1), gamma), wr);
        auto a2 = add(add(mul(x, bk2), gamma), wo);
        stv(A.num, i, mul(mul(mul(a0, a1), a2), fix3()));
        auto b0 = add(add(mul(ldv(A.s1, i), beta261), gamma), wl);
        auto b1 = add(add(mul(ldv(A.s2, i), beta261), gamma), wr);
        auto b2 = add(add(mul(ldv(A.s3, i), beta261), gamma), wo);
        stv(A.den, i, mul(mul(mul(b0, b1), b2), fix3()));
        x = mul(x, step);
    }
}
__global__ void __launch_bounds__(PT) k_z_terms_lanes(const ZTermsArgs* __restrict__ tab) { z_terms_body(tab[blockIdx.y]); } // one table record per lane

// prover.cpp:294-299 and :310-341 fused: the degree-3n part of the quotient numerator on the 4n coset
//   q[i] = (w_l + beta x + gamma)(w_r + beta k1 x + gamma)(w_o + beta k2 x + gamma) zf[i]  -  s1 s2 s3 zf[i + 4],   x = g w_4n^i
// (zf = alpha * Z on the coset, index i + 4 wraps: prover.cpp:286-289 appends the first four values instead)
__device__ __forceinline__ void quotient_large_body(const QuotLargeArgs& A)
{
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n4) return;
    FrM x = pow_tab<true>(A.root, t, A.g_m261);
    const FrC step = cst<true>(A.step_m261), beta = cst<true>(A.beta_m256), bk1 = cst<true>(A.beta_k1_m256), bk2 = cst<true>(A.beta_k2_m256), gamma = cst<true>(A.gamma_m256);
    for (uint32_t i = t; i < A.n4; i += nt) {
        auto t0 = add(add(mul(x, beta), gamma), ldv(A.wl_f, i));
        auto t1 = add(add(mul(x, bk1), gamma), ldv(A.wr_f, i));
        auto t2 = add(add(mul(x, bk2), gamma), ldv(A.wo_f, i));
        FrM id = mul(mul(mul(mul(t0, t1), t2), ldv(A.z_f, i)), fix4());
        FrM pm = mul(mul(mul(mul(ldv(A.s1_f, i), ldv(A.s2_f, i)), ldv(A.s3_f, i)), ldv(A.z_f, (i + 4) & (A.n4 - 1))), fix4());
        stv(A.q, i, sub(id, pm));
        x = mul(x, step);
    }
}
__global__ void __launch_bounds__(PT) k_quotient_large_lanes(const QuotLargeArgs* __restrict__ tab) { quotient_large_body(tab[blockIdx.y]); } // one table record per lane

// prover.cpp:360-402 and arithmetic_widget.cpp:86-101 fused: the degree-2n part on the 2n coset
//   q[i] = (zf[2i+4] - alpha) alpha l1[i+4] + (zf[2i] - alpha) alpha^2 l1[i]
//        + abase (qm wl wr + ql wl + qr wr + qo wo + qc),  wires at index 2i of their 4n transforms
__device__ __forceinline__ void quotient_mid_body(const QuotMidArgs& A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n2) return;
    const uint32_t m4 = 2 * A.n2 - 1, m2 = A.n2 - 1;
    const FrC alpha = cst<true>(A.alpha_m256);
    auto t6 = mul(mul(sub(ldv(A.z_f, (2 * i + 4) & m4), alpha), ldv(A.l1, (i + 4) & m2)), cst<true>(A.alpha_fix_m261));   // * alpha * 2^5
    auto t4 = mul(mul(sub(ldv(A.z_f, 2 * i), alpha), ldv(A.l1, i)), cst<true>(A.alpha2_fix_m261));                          // * alpha^2 * 2^5
    const FrV wl = ldv(A.wl_f, 2 * i), wr = ldv(A.wr_f, 2 * i), wo = ldv(A.wo_f, 2 * i);
    // selector transforms are stored unscaled; abase carries the fix factors: three-operand term needs 2^10, two-operand 2^5
    auto g3 = mul(mul(mul(ldv(A.qm_f, i), wl), wr), cst<true>(A.abase_fix3_m261));
    auto gl = mul(ldv(A.ql_f, i), wl);
    auto gr = mul(ldv(A.qr_f, i), wr);
    auto go = mul(ldv(A.qo_f, i), wo);
    auto g2 = mul(add(add(gl, gr), go), cst<true>(A.abase_fix2_m261));
    auto gc = mul(ldv(A.qc_f, i), cst<true>(A.abase_m261));
    stv(A.q, i, add(add(add(t6, t4), add(g3, g2)), gc));
}
// (second bound = waves per SIMD: holds the body to the registers it takes when its constants arrive as kernel arguments)
__global__ void __launch_bounds__(PT, 6) k_quotient_mid_lanes(const QuotMidArgs* __restrict__ tab) { quotient_mid_body(tab[blockIdx.y]); } // one table record per lane

// mimc_widget.cpp:58-90 on the 4n coset: with T0 = w_o + w_l + q_coef,
//   q[i] += abase q_sel [ (T0^3 - w_r) + alpha (w_r^2 T0 - w_o[i + 4]) ]        (w_o[i + 4] = the next gate's output wire)
__device__ __forceinline__ void quotient_mimc_body(const QuotMimcArgs& A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n4) return;
    const FrV wl = ldv(A.wl_f, i), wr = ldv(A.wr_f, i), wo = ldv(A.wo_f, i), won = ldv(A.wo_f, (i + 4) & (A.n4 - 1));
    const auto t0 = weak(add(add(wo, wl), ldv(A.qcoef_f, i)));
    const auto t0sq = mulv(t0, t0);
    const auto t1 = weak(sub(mulv(t0sq, t0), wr));
    const auto t2 = mul(weak(sub(mulv(mulv(wr, wr), t0), won)), cst<true>(A.alpha_m261));
    const auto sum = weak(add(t1, t2));
    stv(A.q, i, add(mul(mul(sum, ldv(A.qsel_f, i)), cst<true>(A.abase_fix_m261)), ldv(A.q, i)));
}
__global__ void __launch_bounds__(PT, 8) k_quotient_mimc_lanes(const QuotMimcArgs* __restrict__ tab) { quotient_mimc_body(tab[blockIdx.y]); } // one table record per lane

// sequential_widget.cpp:47-62: q[i] += c q_o_next[i] w_o[2i + 4] on the 2n coset (index 2i + 4 of the 4n evaluations = the next gate's row)
__device__ __forceinline__ void quotient_seq_body(const QuotSeqArgs& A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n2) return;
    const uint32_t m4 = 2 * A.n2 - 1;
    auto t = mul(mul(ldv(A.qon_f, i), ldv(A.wo_f, (2 * i + 4) & m4)), cst<true>(A.c_fix_m261));
    stv(A.q, i, add(t, ldv(A.q, i)));
}
__global__ void __launch_bounds__(PT) k_quotient_seq_lanes(const QuotSeqArgs* __restrict__ tab) { quotient_seq_body(tab[blockIdx.y]); } // one table record per lane

// bool_widget.cpp:62-100: q[i] += c_l q_bl (w_l^2 - w_l) + c_r q_br (w_r^2 - w_r) + c_o q_bo (w_o^2 - w_o), wires at index 2i
__device__ __forceinline__ void quotient_bool_body(const QuotBoolArgs& A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n2) return;
    const FrV wl = ldv(A.wl_f, 2 * i), wr = ldv(A.wr_f, 2 * i), wo = ldv(A.wo_f, 2 * i);
    auto tl = mul(mul(weak(sub(mulv(wl, wl), wl)), ldv(A.qbl_f, i)), cst<true>(A.cl_fix_m261));
    auto tr = mul(mul(weak(sub(mulv(wr, wr), wr)), ldv(A.qbr_f, i)), cst<true>(A.cr_fix_m261));
    auto to = mul(mul(weak(sub(mulv(wo, wo), wo)), ldv(A.qbo_f, i)), cst<true>(A.co_fix_m261));
    stv(A.q, i, add(add(add(tl, tr), to), ldv(A.q, i)));
}
__global__ void __launch_bounds__(PT) k_quotient_bool_lanes(const QuotBoolArgs* __restrict__ tab) { quotient_bool_body(tab[blockIdx.y]); } // one table record per lane

// ---- witness check: does the witness satisfy the circuit in rows 0 .. n-2 (include/bbgpu.h, bbgpu_plonk_check_witness) --------------------------------
// A zero test needs no canonical value: a fresh product (or shared-reduction sum of products) has exact limbs and a value below 2p, so it is zero modulo
// r iff it is 0 or r (is_zero_mulout); every identity below ends in such a product, and a constant factor 2^-5k of the Montgomery forms does not move a zero.
//
// The workgroup's findings meet on chip: shuffles inside a wave, four LDS slots across the waves, then ONE thread issues the atomics -- and only if the
// workgroup found anything, so a witness that satisfies the circuit issues none.
__device__ __forceinline__ void check_commit(uint32_t bad, unsigned long long first, uint32_t kinds, unsigned long long* __restrict__ d_count,
                                             unsigned long long* __restrict__ d_first, uint32_t* __restrict__ d_kinds)
{
    __shared__ unsigned long long s_first[PT / 64];
    __shared__ uint32_t s_bad[PT / 64], s_kinds[PT / 64];
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        bad += __shfl_xor(bad, o);
        kinds |= __shfl_xor(kinds, o);
        const uint32_t lo = __shfl_xor((uint32_t)first, o), hi = __shfl_xor((uint32_t)(first >> 32), o);
        const unsigned long long f = ((unsigned long long)hi << 32) | lo;
        first = f < first ? f : first;
    }
    if ((threadIdx.x & 63) == 0) {
        s_bad[threadIdx.x >> 6] = bad;
        s_kinds[threadIdx.x >> 6] = kinds;
        s_first[threadIdx.x >> 6] = first;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < PT / 64; w++) {
        bad += s_bad[w];
        kinds |= s_kinds[w];
        first = s_first[w] < first ? s_first[w] : first;
    }
    if (!bad) return;
    atomicAdd(d_count, (unsigned long long)bad);
    atomicMin(d_first, first);
    if (d_kinds) atomicOr(d_kinds, kinds);
}

// One thread per row, strided.  The identities (arithmetic_widget.cpp:86-101, sequential_widget.cpp:47-62, bool_widget.cpp:62-100, mimc_widget.cpp:68-85) on
// the VALUES: each must vanish on its own.  The widget set is the circuit's, the same for every lane: uniform branches.
__device__ __forceinline__ void check_gates_body(const WitnessCheckArgs& A)
{
    const uint32_t nt = gridDim.x * blockDim.x, rows = A.n - 1;
    const bool has_seq = A.q_on != nullptr, has_bool = A.q_bl != nullptr, has_mimc = A.q_sel != nullptr;
    const FrC one256 = cst<true>(A.one_m256), one261 = fe_from<Fr>(Fr::ONE);
    uint32_t bad = 0, kinds = 0;
    unsigned long long first = ~0ull;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += nt) {
        const FrV wl = ldv(A.w_l, i), wr = ldv(A.w_r, i), wo = ldv(A.w_o, i);
        uint32_t k = 0;
        // q_l w_l + q_r w_r and (q_m w_l) w_r + q_o w_o: two reductions for four products, all carrying 2^251; one more brings the sum to the memory
        // form and adds q_c
        const auto t1 = mul_add(ldv(A.q_l, i), wl, ldv(A.q_r, i), wr);
        const auto t2 = mul_add(mulv(ldv(A.q_m, i), wl), wr, ldv(A.q_o, i), wo);
        const FrV qc = ldv(A.q_c, i);
        bool arith_zero;
        if (has_seq) arith_zero = is_zero_mulout(mul_add(add(add(t1, t2), mul(ldv(A.q_on, i), ldv(A.w_o, i + 1))), fix2(), qc, one261));
        else arith_zero = is_zero_mulout(mul_add(add(t1, t2), fix2(), qc, one261));
        if (!arith_zero) k |= BBGPU_PLONK_FAIL_ARITH;
        if (has_bool) { // q (w^2 - w) = q w (w - 1)
            if (!is_zero_mulout(mul(mul(wl, sub(wl, one256)), ldv(A.q_bl, i)))) k |= BBGPU_PLONK_FAIL_BOOL_L;
            if (!is_zero_mulout(mul(mul(wr, sub(wr, one256)), ldv(A.q_br, i)))) k |= BBGPU_PLONK_FAIL_BOOL_R;
            if (!is_zero_mulout(mul(mul(wo, sub(wo, one256)), ldv(A.q_bo, i)))) k |= BBGPU_PLONK_FAIL_BOOL_O;
        }
        if (has_mimc) { // t = w_o + w_l + q_coef:  q_sel (t^3 - w_r),  q_sel (t w_r^2 - w_o[i + 1])
            const FrV qsel = ldv(A.q_sel, i);
            const auto t = weak(add(add(wo, wl), ldv(A.q_coef, i)));
            if (!is_zero_mulout(mul(weak(sub(mulv(mulv(t, t), t), wr)), qsel))) k |= BBGPU_PLONK_FAIL_MIMC_CUBE;
            if (!is_zero_mulout(mul(weak(sub(mulv(mulv(wr, wr), t), ldv(A.w_o, i + 1))), qsel))) k |= BBGPU_PLONK_FAIL_MIMC_OUT;
        }
        if (k) {
            const unsigned long long f = ((unsigned long long)i << 32) | k;
            first = f < first ? f : first;
            kinds |= k;
            bad++;
        }
    }
    check_commit(bad, first, kinds, &A.counts->gate_failures, &A.first->gate, &A.counts->kinds);
}
__global__ void __launch_bounds__(PT) k_check_gates_lanes(const WitnessCheckArgs* __restrict__ tab) { check_gates_body(tab[blockIdx.y]); } // one table record per lane

// One thread per row: its three mapping entries, decoded as k_sigma_from_mapping decodes them; the value at the target (a 32-byte gather out of the lane's
// three wire vectors) must equal the position's own value modulo r -- the difference is tested, the representatives may differ -- and the target must lie in
// a constrained row.
__device__ __forceinline__ void check_copies_body(const WitnessCheckArgs& A)
{
    const uint32_t nt = gridDim.x * blockDim.x, rows = A.n - 1;
    const FrC one261 = fe_from<Fr>(Fr::ONE);
    uint32_t bad = 0;
    unsigned long long first = ~0ull;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += nt) {
        auto position = [&](const uint32_t* __restrict__ mapping, const uint32_t* __restrict__ own, uint32_t wire) {
            const uint32_t m = mapping[i];
            const uint32_t row = (m & ((1u << 29) - 1u)) & (A.n - 1), type = (m >> 30) & 3u;
            const uint32_t* __restrict__ src = type == 2 ? A.w_o : type == 1 ? A.w_r : A.w_l;
            const bool equal = is_zero_mulout(mul(sub(ldv(own, i), ldv(src, row)), one261));
            if (equal && row < rows) return;
            const unsigned long long f = ((unsigned long long)((i << 2) | wire) << 32) | m;
            first = f < first ? f : first;
            bad++;
        };
        position(A.s1, A.w_l, 0);
        position(A.s2, A.w_r, 1);
        position(A.s3, A.w_o, 2);
    }
    check_commit(bad, first, 0, &A.counts->copy_failures, &A.first->copy, nullptr);
}
__global__ void __launch_bounds__(PT) k_check_copies_lanes(const WitnessCheckArgs* __restrict__ tab) { check_copies_body(tab[blockIdx.y]); } // one table record per lane

// Wires from composer variables: element e of the 3n wire cells (wire-major) is variables[index[e]], copied bit for bit -- no reduction, the wires path
// uploads whatever representative the caller gave.  Two adjacent lanes per element, 16 bytes each: a wave reads 32 consecutive indices (each by both
// lanes of its pair: one 128-byte request), gathers 32 rows of 32 bytes -- the gather k_check_copies_lanes does, out of a vector that sits in L2 / the Infinity
// Cache (2 MiB per lane at 2^16 gates) -- and stores 1 KiB contiguously.  Plain vector loads and stores, nothing else.
__device__ __forceinline__ void expand_wires_body(const ExpandWiresArgs& A)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, e = t >> 1, half = t & 1u;
    if (e >= 3u * A.n) return;
    const uint32_t k = e / A.n, i = e - k * A.n;
    const uint32_t* __restrict__ index = k == 2 ? A.index[2] : k == 1 ? A.index[1] : A.index[0];
    uint32_t* __restrict__ dst = k == 2 ? A.dst[2] : k == 1 ? A.dst[1] : A.dst[0];
    // a defensive clamp: bbgpu_plonk_prover_set_wire_map refused every index >= num_variables on the host, so on an intact map it changes nothing; a map
    // corrupted afterwards gives a wrong value (the witness check or the verifier sees it), not a read outside the variables
    const uint32_t v = min(index[i], A.num_variables - 1u);
    reinterpret_cast<uint4*>(dst + (size_t)i * 8)[half] = reinterpret_cast<const uint4*>(A.variables + (size_t)v * 8)[half];
}
__global__ void __launch_bounds__(PT) k_expand_wires_lanes(const ExpandWiresArgs* __restrict__ tab) { expand_wires_body(tab[blockIdx.y]); } // one table record per lane

// polynomial_arithmetic.cpp:381-476, first half: d[i] = g w_N^i - 1 (to be inverted)
__global__ void __launch_bounds__(PT) k_l1_denominators(uint32_t* __restrict__ d, uint32_t N, PowTab root, Limbs9 g_m256, Limbs9 step_m261)
{
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    FrM x = pow_tab(root, t, g_m256); // memory form
    const FrC step = cst(step_m261), one = fe_from<Fr>(Fr::ONE_M256);
    for (uint32_t i = t; i < N; i += nt) {
        stv(d, i, sub(x, one));
        x = mul(x, step);
    }
}
// second half: l1[i] = inv[i] * ((g^n w_k^(i mod k)) - 1) / n
__global__ void __launch_bounds__(PT) k_l1_scale(uint32_t* __restrict__ l1, uint32_t N, uint32_t k, Limbs9 s0, Limbs9 s1, Limbs9 s2, Limbs9 s3)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t sel = i & (k - 1);
    FrC s;
#pragma unroll
    for (int j = 0; j < NL; j++) s.d[j] = sel == 0 ? s0.d[j] : sel == 1 ? s1.d[j] : sel == 2 ? s2.d[j] : s3.d[j];
    stv(l1, i, mul(ldv(l1, i), s));
}

// ---- evaluation and opening in evaluation form (bary_open below; the reference has no counterpart) ----------------------------------------------------
// d[y][i] = z_y - w^i (to be inverted), and one at i == m_y: the index of z_y on the domain, or none (m_y >= n); point y = blockIdx.y, point-major
__global__ void __launch_bounds__(PT) k_bary_denominators(uint32_t* __restrict__ d, uint32_t n, BaryPoints P, PowTab root, Limbs9 step_m261)
{
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    d += (size_t)blockIdx.y * n * 8;
    const uint32_t m = P.m[blockIdx.y];
    Limbs9 one256;
#pragma unroll
    for (int k = 0; k < NL; k++) one256.d[k] = Fr::ONE_M256[k];
    FrM x = pow_tab(root, t, one256); // memory form
    const FrC step = cst(step_m261), z = cst(P.z_m256[blockIdx.y]), one = fe_from<Fr>(Fr::ONE_M256);
    for (uint32_t i = t; i < n; i += nt) {
        if (i == m) stv(d, i, one);
        else stv(d, i, sub(z, x));
        x = mul(x, step);
    }
}
// partial[y][block] = the workgroup's share of sum_i a_i x_i over polynomial y (blockIdx.y), thread t owning i = t, t + T, ...:
//   off the domain (m >= n)  a = v,  x_i = w^i inv_i      (start_m261 = 2^5: the factor a product of three memory-form values lacks)
//   on it                    a = q,  x_i = w^(i - m), the term i == m left out      (start_m261 = w^-m)
// One shared reduction per term: acc <- t x + acc * 1 keeps the (1, 2) bound of a fresh product.
__global__ void __launch_bounds__(PT) k_bary_dot(const uint32_t* __restrict__ a, size_t stride, const uint32_t* __restrict__ inv, uint32_t n, uint32_t m,
                                                 PowTab root, Limbs9 start_m261, Limbs9 step_m261, uint32_t* __restrict__ partial)
{
    __shared__ uint32_t sh[NL * PT];
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    a += (size_t)blockIdx.y * stride * 8;
    const FrC one = fe_from<Fr>(Fr::ONE);
    FrM acc = mul(fe_zero<Fr>(), one);
    if (t < n) {
        FrM x = pow_tab(root, t, start_m261);
        const FrC step = cst(step_m261);
        if (m >= n) {
            for (uint32_t i = t; i < n; i += nt) {
                acc = mul_add(mul(ldv(a, i), ldv(inv, i)), x, acc, one);
                x = mul(x, step);
            }
        } else {
            for (uint32_t i = t; i < n; i += nt) {
                if (i != m) acc = mul_add(ldv(a, i), x, acc, one);
                x = mul(x, step);
            }
        }
    }
    block_sum(partial, (size_t)blockIdx.y * gridDim.x + blockIdx.x, acc, sh);
}
// one workgroup per polynomial: the sum of its partials times c, to slot[y] (off the domain: c = (z^n - 1) / n, the value f(z)) or to element m of the
// quotient (on it: c = -1); sums: batch x 32 bytes of workspace
__global__ void __launch_bounds__(PT) k_bary_finish(const uint32_t* __restrict__ partial, uint32_t blocks, uint32_t* __restrict__ sums, Limbs9 c_m261,
                                                    uint32_t* __restrict__ dst, size_t dst_stride, uint32_t dst_index)
{
    __shared__ uint32_t sh[NL * PT];
    const uint32_t y = blockIdx.x;
    sum_small_body(partial + (size_t)y * blocks * 8, blocks, sums + (size_t)y * 8, sh);
    if (threadIdx.x == 0) stv(dst + (size_t)y * dst_stride * 8, dst_index, mul(ldv(sums, y), cst(c_m261))); // its own store, read back
}
// q[i] = (slot[y] - v[i]) inv[i]; on the domain element m is k_bary_finish's.  q may be v: every element is read by the thread that writes it
__global__ void __launch_bounds__(PT) k_bary_quotient(const uint32_t* v, uint32_t* q, size_t stride, const uint32_t* __restrict__ inv,
                                                      const uint32_t* __restrict__ slot, uint32_t n, uint32_t m)
{
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    v += (size_t)blockIdx.y * stride * 8;
    q += (size_t)blockIdx.y * stride * 8;
    const FrV y = ldv(slot, blockIdx.y);
    for (uint32_t i = t; i < n; i += nt)
        if (i != m) stv(q, i, mulv(sub(y, ldv(v, i)), ldv(inv, i)));
}
// F_i = sum_b gamma_b v_{b,i} over `batch` polynomials `stride` elements apart (gamma by value, 2^261 form): one shared reduction per term, memory form
__device__ __forceinline__ FrM fold_at(const uint32_t* __restrict__ v, size_t stride, int batch, const FoldCoeffs& G, uint32_t i)
{
    const FrC one = fe_from<Fr>(Fr::ONE);
    FrM f = mul(ldv(v, i), cst(G.c[0]));
    for (int b = 1; b < batch; b++) f = mul_add(ldv(v + (size_t)b * stride * 8, i), cst(G.c[b]), f, one);
    return f;
}
// out[i] = F_i, or out[i] + F_i (bbgpu_fr_fold_device; the fold of an opening at z on the domain)
__global__ void __launch_bounds__(PT) k_fold(uint32_t* __restrict__ out, const uint32_t* __restrict__ v, size_t stride, int batch, FoldCoeffs G, uint32_t n,
                                             uint32_t accumulate)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const FrM f = fold_at(v, stride, batch, G, i);
    if (accumulate) stv(out, i, add(f, ldv(out, i)));
    else stv(out, i, f);
}
// the fold and k_bary_dot's sum off the domain in one trip over the values: folded[i] = F_i and partial[block] = the workgroup's share of
// sum_i F_i w^i inv_i, thread t owning i = t, t + T, ... (start_m261 = 2^5, as in k_bary_dot)
__global__ void __launch_bounds__(PT) k_bary_fold_dot(const uint32_t* __restrict__ v, size_t stride, int batch, FoldCoeffs G, const uint32_t* __restrict__ inv,
                                                      uint32_t n, PowTab root, Limbs9 start_m261, Limbs9 step_m261, uint32_t* __restrict__ folded,
                                                      uint32_t* __restrict__ partial)
{
    __shared__ uint32_t sh[NL * PT];
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    const FrC one = fe_from<Fr>(Fr::ONE);
    FrM acc = mul(fe_zero<Fr>(), one);
    if (t < n) {
        FrM x = pow_tab(root, t, start_m261);
        const FrC step = cst(step_m261);
        for (uint32_t i = t; i < n; i += nt) {
            const FrM f = fold_at(v, stride, batch, G, i);
            stv(folded, i, f);
            acc = mul_add(mul(f, ldv(inv, i)), x, acc, one);
            x = mul(x, step);
        }
    }
    block_sum(partial, blockIdx.x, acc, sh);
}

// prover.cpp:520-528 + arithmetic_widget.cpp:106-126: r[i] = sum_j c_j p_j[i] over the seven coefficient-form polynomials
__device__ __forceinline__ void lincomb_body(const LinCombArgs& A)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    FrM acc = mul(ldv(A.p[0], i), cst<true>(A.c[0]));
    for (int j = 1; j < A.count; j++) acc = tight2<Fr>(add(acc, mul(ldv(A.p[j], i), cst<true>(A.c[j]))));
    if (A.out_add) acc = tight2<Fr>(add(acc, ldv(A.out_add, i)));
    stv(A.out, i, acc);
}
__global__ void __launch_bounds__(PT) k_lincomb_lanes(const LinCombArgs* __restrict__ tab) { lincomb_body(tab[blockIdx.y]); } // one table record per lane

// ---- lane-batched forms of the small kernels (blockIdx.y = record of a device table, or lane of a strided vector) ------------------------------------
// prover.cpp:253-269: dst (4n) = beta sigma(X) + w(X) + gamma in coefficient form, zero-padded
__global__ void __launch_bounds__(PT) k_sigma_prepare_lanes(const SigmaPrepArgs* __restrict__ tab)
{
    const SigmaPrepArgs& A = tab[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_dst) return;
    if (i >= A.n) {
        uint4* q = reinterpret_cast<uint4*>(A.dst + (size_t)i * 8);
        q[0] = make_uint4(0, 0, 0, 0);
        q[1] = make_uint4(0, 0, 0, 0);
        return;
    }
    auto v = add(ldv(A.sigma, i), ldv(A.w, i));
    if (i == 0) stv(A.dst, i, add(v, cst<true>(A.gamma_m256)));
    else stv(A.dst, i, v);
}
__global__ void __launch_bounds__(PT) k_add_inplace_lanes(uint32_t* __restrict__ a, size_t stride_a, const uint32_t* __restrict__ b, size_t stride_b, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    a += (size_t)blockIdx.y * stride_a * 8;
    b += (size_t)blockIdx.y * stride_b * 8;
    stv(a, i, add(ldv(a, i), ldv(b, i)));
}
// polynomial_arithmetic.cpp:478-560: c[i] *= (x_i - w_n^-1) / ((x_i)^n - 1),  x_i = g w_N^i;  (x_i)^n - 1 takes k = N/n values
__global__ void __launch_bounds__(PT) k_divide_vanishing_lanes(uint32_t* __restrict__ c, size_t stride, uint32_t N, uint32_t k, PowTab root, Limbs9 g_m261,
                                                             Limbs9 step_m261, Limbs9 wninv_m261, Limbs9 inv0, Limbs9 inv1, Limbs9 inv2, Limbs9 inv3)
{
    const uint32_t nt = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    c += (size_t)blockIdx.y * stride * 8;
    FrM x = pow_tab(root, t, g_m261);
    const FrC step = cst(step_m261), wninv = cst(wninv_m261);
    const uint32_t sel = t & (k - 1); // nt is a multiple of 4, so i mod k is fixed per thread
    const FrC iv = cst(sel == 0 ? inv0 : sel == 1 ? inv1 : sel == 2 ? inv2 : inv3);
    for (uint32_t i = t; i < N; i += nt) {
        auto num = weak(sub(x, wninv)); // 2^261 form
        stv(c, i, mul(mul(ldv(c, i), num), iv));
        x = mul(x, step);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static inline uint32_t pw_blocks(size_t n) { return (uint32_t)((n + PT - 1) / PT); }
// grid for the strided kernels: a multiple of 4 threads in total, at most 1024 workgroups
static inline uint32_t strided_blocks(size_t n)
{
    size_t b = (n + 4 * PT - 1) / (4 * PT);
    return (uint32_t)std::min<size_t>(std::max<size_t>(b, 1), 1024);
}

PowTab make_powtab(const host::Fr& base)
{
    PowTab T;
    host::Fr b = base;
    for (int j = 0; j < 24; j++) {
        T.p[j] = host::limbs_m261(b);
        b = host::fr_sqr(b);
    }
    return T;
}

int Scratch::ensure(size_t bytes)
{
    if (bytes <= cap) return BBGPU_OK;
    if (base) (void)dev_free(base);
    base = nullptr;
    cap = 0;
    HIPCHK(dev_malloc((void**)&base, bytes));
    cap = bytes;
    return BBGPU_OK;
}
void Scratch::release()
{
    if (base) (void)dev_free(base);
    if (h_pinned) (void)hipHostFree(h_pinned);
    base = nullptr;
    h_pinned = nullptr;
    cap = 0;
}
static int ensure_pinned(Scratch& S)
{
    if (!S.h_pinned) HIPCHK(hipHostMalloc((void**)&S.h_pinned, 4096));
    return BBGPU_OK;
}

int powers(uint64_t* d_out, size_t n, const host::Fr& base, const host::Fr& start, hipStream_t st)
{
    const uint32_t blocks = strided_blocks(n);
    k_powers<<<blocks, PT, 0, st>>>((uint32_t*)d_out, (uint32_t)n, make_powtab(base), host::limbs_m256(start),
                                   host::limbs_m261(host::fr_pow(base, (uint64_t)blocks * PT)));
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int copy_pad(uint64_t* d_dst, const uint64_t* d_src, size_t n_src, size_t n_dst, hipStream_t st)
{
    CopyPadArgs A{}; // the unscaled record
    A.dst = (uint32_t*)d_dst;
    A.src = (const uint32_t*)d_src;
    A.n_src = (uint32_t)n_src;
    A.n_dst = (uint32_t)n_dst;
    k_copy_pad<<<pw_blocks(n_dst), PT, 0, st>>>(A);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int mul_pointwise(uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n, hipStream_t st)
{
    k_mul<<<pw_blocks(n), PT, 0, st>>>((uint32_t*)d_out, (const uint32_t*)d_a, (const uint32_t*)d_b, (uint32_t)n);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
static int mul2c(uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n, const host::Fr& c, hipStream_t st)
{
    const host::Fr cf = host::fr_mul(c, host::fr_from_u64(32)); // c * 2^5: the FIX2 factor folded in
    k_mul2c<<<pw_blocks(n), PT, 0, st>>>(Mul2cArgs{ (uint32_t*)d_out, (const uint32_t*)d_a, (const uint32_t*)d_b, (uint32_t)n, host::limbs_m261(cf) });
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// scratch layout of a scan over n elements: tpart, bpart, bcarry, plus the nested single-block scan's own tpart/bpart -- and, above 2^22 elements,
// where the scan over the block totals is a two-level scan of its own, that scan's scratch behind it
static size_t scan_scratch_own(size_t n)
{
    const size_t nt = (n + RUN - 1) / RUN, nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    return (((nt + 2 * nb + (nb + RUN - 1) / RUN + 8) * 32 + 1024) + 255) & ~(size_t)255;
}
size_t scan_scratch_bytes(size_t n)
{
    const size_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    return scan_scratch_own(n) + (nb > (size_t)SCAN_BLOCK ? scan_scratch_bytes(nb) : 0);
}

// MODE 0 product scan (z ignored) / MODE 1 Horner suffix sums with multiplier z.  Three phases: runs of RUN per thread and a scan of the thread partials
// in LDS (phase 1), a scan over the block totals, the carry pass (phase 3).  The scan over the block totals takes one of three forms:
//   fused   (<= SCAN_T block totals, n <= 2^19): every workgroup of phase 3 scans them for itself; two launches;
//   one workgroup (<= SCAN_BLOCK block totals, n <= 2^22): phase 1 and phase 3 of a second level B, one workgroup per job; four launches;
//   nested  (above, n up to 2^28, the transforms' limit; the prover's L_1 scan is 2n): the same three phases again, on the scratch behind this level's.
// The plan of one job: A (phase 1), B (the one-workgroup level over the block totals) and A3 (phase 3) in the job's scratch at `base`.  The total of
// everything is the one element B.bpart points at -- the caller's slot where it gave one -- whichever form writes it.
static void scan_plan(int mode, const ScanJob& J, uint8_t* base, ScanArgs& A, ScanArgs& B, ScanArgs& A3)
{
    const size_t n = J.n;
    const size_t nt = (n + RUN - 1) / RUN, nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK, nt2 = (nb + RUN - 1) / RUN;
    uint32_t* tpart = (uint32_t*)base;
    uint32_t* bpart = tpart + nt * 8;
    uint32_t* bcarry = bpart + nb * 8;
    uint32_t* tpart2 = bcarry + nb * 8;
    uint32_t* bpart2 = tpart2 + nt2 * 8; // one element: the grand total
    A = ScanArgs{};
    A.in = (const uint32_t*)J.in;
    A.out = (uint32_t*)J.out;
    A.tpart = tpart;
    A.bpart = bpart;
    A.bcarry = bcarry;
    A.n = (uint32_t)n;
    A.reverse = J.reverse ? 1u : 0u;
    A.inclusive = J.inclusive ? 1u : 0u;
    A.has_carry = 1;
    B = A; // the scan over the block totals: exclusive, same direction
    B.in = bpart;
    B.out = bcarry;
    B.tpart = tpart2;
    B.bpart = J.d_total ? (uint32_t*)J.d_total : bpart2;
    B.bcarry = nullptr;
    B.has_carry = 0;
    B.n = (uint32_t)nb;
    B.inclusive = 0;
    if (mode == 1) {
        host::Fr zr = host::fr_pow(J.z, RUN);
        host::Fr p = zr;
        for (int j = 0; j < 8; j++) { A.zpow[j] = host::limbs_m261(p); p = host::fr_sqr(p); }
        A.zpow[8] = host::limbs_m261(J.z);
        A.zpow[9] = host::limbs_m261(zr);
        // the level over the block totals: its "elements" are whole blocks, so its z is z^SCAN_BLOCK
        host::Fr zb = host::fr_pow(J.z, SCAN_BLOCK);
        p = zb;
        for (int j = 0; j < 8; j++) { A.zpow[12 + j] = host::limbs_m261(p); p = host::fr_sqr(p); }
        host::Fr zbr = host::fr_pow(zb, RUN);
        p = zbr;
        for (int j = 0; j < 8; j++) { B.zpow[j] = host::limbs_m261(p); p = host::fr_sqr(p); }
        B.zpow[8] = host::limbs_m261(zb);
        B.zpow[9] = host::limbs_m261(zbr);
    }
    A3 = A;
    if (nb <= (size_t)SCAN_T) { // fused: phase 3 also runs for a scan without an output vector, for the total
        A3.fused_nb = (uint32_t)nb;
        A3.total_out = B.bpart;
    } else if (!J.out) {
        A3.n = 0;
    }
}
// How a phase is launched is all that tells a single scan from the scans of a lane table: its record by value, or every job's record from the table
// (dev, grid.y = job).
template <int MODE> static void scan_phase1(const ScanArgs* rec, const ScanArgs* dev, dim3 grid, hipStream_t st)
{
    if (dev) k_scan_phase1_tab<MODE><<<grid, SCAN_T, 0, st>>>(dev);
    else k_scan_phase1<MODE><<<grid, SCAN_T, 0, st>>>(*rec);
}
template <int MODE> static void scan_phase3(const ScanArgs* rec, const ScanArgs* dev, dim3 grid, hipStream_t st)
{
    if (dev) k_scan_phase3_tab<MODE><<<grid, SCAN_T, 0, st>>>(dev);
    else k_scan_phase3<MODE><<<grid, SCAN_T, 0, st>>>(*rec);
}
// `count` scans of one length n >= 1, job j on the scratch at base + j * scan_scratch_bytes(n) (the caller has made it large enough: the whole nest at
// once, the workspace must not move under the launches of an outer level).  T: the lane table that carries the records; null: one job, by value.
template <int MODE> static int scan_issue(const ScanJob* jobs, int count, uint8_t* base, LaneTable* T, hipStream_t st)
{
    const size_t n = jobs[0].n, nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK, per = scan_scratch_bytes(n);
    ScanArgs one[3];
    ScanArgs *A = &one[0], *B = &one[1], *A3 = &one[2];
    const ScanArgs *dA = nullptr, *dB = nullptr, *dA3 = nullptr;
    if (T) {
        if (int rc = T->push(count, &A, &dA)) return rc;
        if (int rc = T->push(count, &B, &dB)) return rc;
        if (int rc = T->push(count, &A3, &dA3)) return rc;
    }
    bool any_out = false;
    for (int j = 0; j < count; j++) {
        scan_plan(MODE, jobs[j], base + per * (size_t)j, A[j], B[j], A3[j]);
        any_out = any_out || jobs[j].out;
    }
    if (T)
        if (int rc = T->flush(st)) return rc;
    const dim3 g1((uint32_t)nb, count), gb(1, count);
    scan_phase1<MODE>(A, dA, g1, st);
    if (nb > (size_t)SCAN_BLOCK) {
        // more block totals than one workgroup scans: the scan over them (exclusive, same direction; Horner: multiplier z^SCAN_BLOCK) is a scan of this
        // kind itself, run on the scratch behind this level's; its grand total lands where the one-workgroup form leaves it (B.bpart).  One job only.
        ScanJob I{};
        I.in = (const uint64_t*)A[0].bpart;
        I.out = (uint64_t*)A[0].bcarry;
        I.n = nb;
        I.reverse = jobs[0].reverse;
        I.inclusive = false;
        I.d_total = (uint64_t*)B[0].bpart;
        if (MODE == 1) I.z = host::fr_pow(jobs[0].z, SCAN_BLOCK);
        if (int rc = scan_issue<MODE>(&I, 1, base + scan_scratch_own(n), nullptr, st)) return rc;
    } else if (nb > (size_t)SCAN_T) {
        scan_phase1<MODE>(B, dB, gb, st);
        scan_phase3<MODE>(B, dB, gb, st);
    }
    if (nb <= (size_t)SCAN_T || any_out) scan_phase3<MODE>(A3, dA3, g1, st);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
static int scan_run(int mode, const uint64_t* d_in, uint64_t* d_out, size_t n, bool reverse, bool inclusive, const host::Fr* z, Scratch& S,
                    hipStream_t st, uint64_t* d_total /* optional: 32-byte device slot receiving the full combination */)
{
    if (n == 0) return BBGPU_OK;
    if (n > ((size_t)1 << 28)) {
        set_error("scan of %zu elements: at most 2^28", n);
        return BBGPU_ERR_SIZE;
    }
    ScanJob J{};
    J.in = d_in; J.out = d_out; J.n = n; J.reverse = reverse; J.inclusive = inclusive; J.d_total = d_total;
    if (z) J.z = *z;
    if (int rc = S.ensure(scan_scratch_bytes(n) + 64)) return rc;
    return mode == 0 ? scan_issue<0>(&J, 1, S.base, nullptr, st) : scan_issue<1>(&J, 1, S.base, nullptr, st);
}
int scan_lanes(int mode, const ScanJob* jobs, int count, LaneTable& T, Scratch& S, hipStream_t st)
{
    if (count < 1) return BBGPU_ERR_ARG;
    const size_t n = jobs[0].n;
    for (int j = 0; j < count; j++)
        if (jobs[j].n != n || n == 0 || n > (size_t)SCAN_BLOCK * SCAN_BLOCK) { // the nested form is not batched
            set_error("lane-batched scan: one length for all jobs, 1 <= n <= 2^22");
            return BBGPU_ERR_SIZE;
        }
    if (int rc = S.ensure(scan_scratch_bytes(n) * (size_t)count + 64)) return rc;
    return mode == 0 ? scan_issue<0>(jobs, count, S.base, &T, st) : scan_issue<1>(jobs, count, S.base, &T, st);
}

int product_scan(const uint64_t* d_in, uint64_t* d_out, size_t n, bool reverse, bool inclusive, Scratch& S, hipStream_t st, uint64_t* d_total)
{
    return scan_run(0, d_in, d_out, n, reverse, inclusive, nullptr, S, st, d_total);
}
int horner_suffix(const uint64_t* d_in, uint64_t* d_out, size_t n, const host::Fr& z, bool inclusive, Scratch& S, hipStream_t st, uint64_t* d_total)
{
    return scan_run(1, d_in, d_out, n, true, inclusive, &z, S, st, d_total);
}

// polynomial_arithmetic::evaluate (:337-373): result left in a 32-byte device slot (canonical); evaluate() also fetches it
// workgroups of an evaluation: every lane pays ~log2(lanes) multiplications for its z^t on top of one per coefficient, so a lane takes
// 8 coefficients (Horner in z^T) before the grid grows: at n = 2^16 one lane per coefficient cost 17 dependent multiplications each
// (the prover's seven openings: 73 us), 8 per lane cost 8 + 13 for eight (21 us)
static uint32_t eval_blocks(size_t n)
{
    return (uint32_t)std::min<size_t>(std::max<size_t>((n + (size_t)PT * 8 - 1) / ((size_t)PT * 8), 1), 256);
}
int evaluate_to_device(const uint64_t* d_coeffs, size_t n, const host::Fr& z, uint64_t* d_result, Scratch& S, hipStream_t st)
{
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_result, 0, 32, st));
        return BBGPU_OK;
    }
    const uint32_t blocks = eval_blocks(n);
    int rc = S.ensure((size_t)blocks * 32 + 64);
    if (rc) return rc;
    const uint32_t nt = blocks * PT;
    k_eval_partial<<<blocks, PT, 0, st>>>((const uint32_t*)d_coeffs, (uint32_t)n, make_powtab(z), host::limbs_m261(host::fr_pow(z, nt)), (uint32_t*)S.base);
    k_sum_small<<<1, PT, 0, st>>>((const uint32_t*)S.base, blocks, (uint32_t*)d_result);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int evaluate(const uint64_t* d_coeffs, size_t n, const host::Fr& z, host::Fr* out, Scratch& S, hipStream_t st)
{
    int rc = ensure_pinned(S);
    if (rc) return rc;
    rc = S.ensure(((n + PT - 1) / PT + 8) * 32 + 128);
    if (rc) return rc;
    // the partials live at the start of the scratch; the result slot sits past them
    const size_t slot_off = (std::min<size_t>((n + PT - 1) / PT, 256) + 1) * 32;
    uint64_t* d_res = (uint64_t*)(S.base + slot_off);
    rc = evaluate_to_device(d_coeffs, n, z, d_res, S, st);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(S.h_pinned, d_res, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out->d, S.h_pinned, 32);
    return BBGPU_OK;
}

// fr::batch_invert (field.hpp:503-522) on a resident vector: inv(a_i) = (prod_{j<i} a_j)(prod_{j>i} a_j) / prod_j a_j.
// Two product scans and ONE field inversion on the host (10 us; a Fermat chain on one GPU lane takes ~0.25 ms).
// d_tmp: n elements of workspace.  All a_i must be non-zero (the reference's loop has the same precondition).
int batch_invert(uint64_t* d_v, uint64_t* d_tmp, size_t n, Scratch& S, hipStream_t st)
{
    if (n == 0) return BBGPU_OK;
    int rc = ensure_pinned(S);
    if (rc) return rc;
    const size_t off_suffix = (scan_scratch_bytes(n) + 64 + 63) & ~(size_t)63;
    rc = S.ensure(off_suffix + n * 32 + 64);
    if (rc) return rc;
    uint64_t* d_suffix = (uint64_t*)(S.base + off_suffix);
    uint64_t* d_total = d_suffix + n * 4; // 32 bytes past the suffix array
    rc = product_scan(d_v, d_tmp, n, false, false, S, st, d_total); // exclusive prefix products -> d_tmp, total
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(S.h_pinned, d_total, 32, hipMemcpyDeviceToHost, st));
    rc = product_scan(d_v, d_suffix, n, true, false, S, st, nullptr); // exclusive suffix products
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(st));
    host::Fr total;
    memcpy(total.d, S.h_pinned, 32);
    rc = mul2c(d_v, d_tmp, d_suffix, n, host::fr_inv(total), st);
    return rc;
}

int sigma_from_mapping(uint64_t* d_out, const uint32_t* d_mapping, const uint64_t* d_roots, size_t n, hipStream_t st)
{
    k_sigma_from_mapping<<<pw_blocks(n), PT, 0, st>>>((uint32_t*)d_out, d_mapping, (const uint32_t*)d_roots, (uint32_t)n,
                                                     host::limbs_m261(host::fr_from_limbs(FrHostP::GEN5)), host::limbs_m261(host::fr_from_limbs(FrHostP::GEN7)));
    HIPCHK(launch_check());
    return BBGPU_OK;
}

static void z_terms_challenges(ZTermsArgs& A, const host::Fr& beta, const host::Fr& gamma)
{
    A.beta_m256 = host::limbs_m256(beta);
    A.beta_m261 = host::limbs_m261(beta);
    A.beta_k1_m256 = host::limbs_m256(host::fr_mul(beta, host::fr_from_limbs(FrHostP::GEN5)));
    A.beta_k2_m256 = host::limbs_m256(host::fr_mul(beta, host::fr_from_limbs(FrHostP::GEN7)));
    A.gamma_m256 = host::limbs_m256(gamma);
}
static void quotient_large_challenges(QuotLargeArgs& A, const host::Fr& beta, const host::Fr& gamma)
{
    A.beta_m256 = host::limbs_m256(beta);
    A.beta_k1_m256 = host::limbs_m256(host::fr_mul(beta, host::fr_from_limbs(FrHostP::GEN5)));
    A.beta_k2_m256 = host::limbs_m256(host::fr_mul(beta, host::fr_from_limbs(FrHostP::GEN7)));
    A.gamma_m256 = host::limbs_m256(gamma);
}
static void quotient_mid_challenges(QuotMidArgs& A, const host::Fr& alpha, const host::Fr& alpha_base)
{
    const host::Fr f2 = host::fr_from_u64(32), f3 = host::fr_from_u64(1024);
    A.alpha_m256 = host::limbs_m256(alpha);
    A.alpha_fix_m261 = host::limbs_m261(host::fr_mul(alpha, f2));
    A.alpha2_fix_m261 = host::limbs_m261(host::fr_mul(host::fr_sqr(alpha), f2));
    A.abase_m261 = host::limbs_m261(alpha_base);
    A.abase_fix2_m261 = host::limbs_m261(host::fr_mul(alpha_base, f2));
    A.abase_fix3_m261 = host::limbs_m261(host::fr_mul(alpha_base, f3));
}
// the records of `lanes` lanes, consecutive from counts / first: zero the counts, all ones (= none) into the atomicMin words
static int check_witness_preset(WitnessCheckCounts* counts, WitnessCheckFirst* first, int lanes, hipStream_t st)
{
    HIPCHK(hipMemsetAsync(counts, 0, sizeof(WitnessCheckCounts) * (size_t)lanes, st));
    HIPCHK(hipMemsetAsync(first, 0xff, sizeof(WitnessCheckFirst) * (size_t)lanes, st));
    return BBGPU_OK;
}
// g^n for n = 2^log2n
static host::Fr coset_gen_pow_n(int log2n)
{
    host::Fr a = host::fr_from_limbs(FrHostP::GEN5);
    for (int i = 0; i < log2n; i++) a = host::fr_sqr(a);
    return a;
}

// divide_by_pseudo_vanishing_polynomial(coeffs, src = 2^log2n, target = 2^log2N), in place on the resident coset evaluations
int divide_by_pseudo_vanishing_lanes(uint64_t* d_coeffs, size_t stride, int lanes, int log2n, int log2N, hipStream_t st)
{
    const int lk = log2N - log2n;
    if (lk < 0 || lk > 2) {
        set_error("divide_by_pseudo_vanishing: target / source domain ratio must be 1, 2 or 4");
        return BBGPU_ERR_SIZE;
    }
    const uint32_t k = 1u << lk;
    const size_t N = (size_t)1 << log2N;
    // (g w_N^i)^n - 1 = g^n w_k^(i mod k) - 1  (compute_multiplicative_subgroup, :104-127)
    host::Fr sub[4], acc = coset_gen_pow_n(log2n), wk = host::fr_root_of_unity(lk);
    Limbs9 inv[4];
    for (uint32_t j = 0; j < 4; j++) {
        if (j < k) {
            sub[j] = host::fr_inv(host::fr_sub(acc, host::fr_one()));
            acc = host::fr_mul(acc, wk);
        } else {
            sub[j] = host::fr_zero();
        }
        inv[j] = host::limbs_m261(sub[j]);
    }
    const host::Fr rootN = host::fr_root_of_unity(log2N), wninv = host::fr_inv(host::fr_root_of_unity(log2n));
    const uint32_t blocks = strided_blocks(N);
    k_divide_vanishing_lanes<<<dim3(blocks, lanes), PT, 0, st>>>((uint32_t*)d_coeffs, stride, (uint32_t)N, k, make_powtab(rootN),
                                                                host::limbs_m261(host::fr_from_limbs(FrHostP::GEN5)),
                                                                host::limbs_m261(host::fr_pow(rootN, (uint64_t)blocks * PT)), host::limbs_m261(wninv), inv[0],
                                                                inv[1], inv[2], inv[3]);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int divide_by_pseudo_vanishing(uint64_t* d_coeffs, int log2n, int log2N, hipStream_t st)
{
    return divide_by_pseudo_vanishing_lanes(d_coeffs, 0, 1, log2n, log2N, st); // a single vector is one lane
}

// compute_lagrange_polynomial_fft(l_1, src = 2^log2n, target = 2^log2N): N resident values; d_tmp: N elements of workspace
int lagrange_l1_fft(uint64_t* d_l1, uint64_t* d_tmp, int log2n, int log2N, Scratch& S, hipStream_t st)
{
    const int lk = log2N - log2n;
    if (lk < 0 || lk > 2) {
        set_error("lagrange_l1_fft: target / source domain ratio must be 1, 2 or 4");
        return BBGPU_ERR_SIZE;
    }
    const uint32_t k = 1u << lk;
    const size_t N = (size_t)1 << log2N;
    const host::Fr rootN = host::fr_root_of_unity(log2N);
    const uint32_t blocks = strided_blocks(N);
    k_l1_denominators<<<blocks, PT, 0, st>>>((uint32_t*)d_l1, (uint32_t)N, make_powtab(rootN), host::limbs_m256(host::fr_from_limbs(FrHostP::GEN5)),
                                            host::limbs_m261(host::fr_pow(rootN, (uint64_t)blocks * PT)));
    HIPCHK(launch_check());
    int rc = batch_invert(d_l1, d_tmp, N, S, st);
    if (rc) return rc;
    // numerators ((g w)^n - 1) / n: k values
    host::Fr acc = coset_gen_pow_n(log2n), wk = host::fr_root_of_unity(lk);
    const host::Fr ninv = host::fr_inv(host::fr_from_u64((uint64_t)1 << log2n));
    Limbs9 s[4];
    for (uint32_t j = 0; j < 4; j++) {
        host::Fr v = host::fr_zero();
        if (j < k) {
            v = host::fr_mul(host::fr_sub(acc, host::fr_one()), ninv);
            acc = host::fr_mul(acc, wk);
        }
        s[j] = host::limbs_m261(v);
    }
    k_l1_scale<<<pw_blocks(N), PT, 0, st>>>((uint32_t*)d_l1, (uint32_t)N, k, s[0], s[1], s[2], s[3]);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// Evaluation and opening of `batch` polynomials given by their values on the size-2^log2n domain (polynomial b at d_values + b * stride elements), at one
// z (canonical; on_domain / m: the host's verdict, host_lagrange_open.hpp).  ONE inversion for the whole batch: the denominators z - w^i are shared.
//   off the domain   denominators, batch_invert, dot (v_i w^i inv_i), finish (* (z^n - 1) / n -> slot b), quotient (slot b - v_i) inv_i
//   on it            denominators (one at m), batch_invert, v_m -> slot b by a copy, quotient (all but m), dot (q_i w^(i - m)), finish (* -1 -> q_m);
//                    without a quotient only the copy
// bary_open is "make inverses" (bary_inverses) followed by "use inverses" (bary_apply); an opening session makes the inverses of several points once
// and uses them call by call (bary_open_with, bary_open_folded).
// d_quotient: null (evaluation only), d_values itself, or a buffer that does not overlap it.  h_out: null, or batch values read back (the only
// synchronisation besides batch_invert's).  d_tmp: n elements.  The scratch holds batch_invert's share first, then the inverses, the partials and the slots.
// slot b = element m of polynomial b, as it stands
static hipError_t bary_stash(uint32_t* d_slot, const uint64_t* d_vm, size_t stride, int batch, hipStream_t st)
{
    if (batch > 1 && stride * 32 <= 0x7fffffffu) // one strided copy while the pitch is one the runtime takes
        return hipMemcpy2DAsync(d_slot, 32, d_vm, stride * 32, 32, (size_t)batch, hipMemcpyDeviceToDevice, st);
    for (int b = 0; b < batch; b++)
        if (hipError_t e = hipMemcpyAsync(d_slot + 8 * (size_t)b, d_vm + 4 * (size_t)b * stride, 32, hipMemcpyDeviceToDevice, st)) return e;
    return hipSuccess;
}
// batch x 4 words from the slots to the host: the read-back and the synchronisation of a call that returns values
static int bary_read_slots(const uint32_t* d_slot, int batch, host::Fr* h_out, Scratch& S, hipStream_t st)
{
    HIPCHK(d2h_async(S.h_pinned, d_slot, (size_t)batch * 32, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int b = 0; b < batch; b++) {
        host::Fr y;
        memcpy(y.d, (const uint8_t*)S.h_pinned + 32 * (size_t)b, 32);
        h_out[b] = host::fr_mul(y, host::fr_one()); // v_m is the caller's representative: canonical out
    }
    return BBGPU_OK;
}
// what the kernels behind the inversion work in: the dot kernel's partials, the slots and the sums of `batch` polynomials
struct BaryWork {
    uint32_t *partial, *slot, *sums;
};
static size_t bary_work_bytes(size_t n, int batch) { return ((size_t)batch * eval_blocks(n) + 2 * (size_t)batch) * 32; }
static BaryWork bary_work_at(uint8_t* base, size_t n, int batch)
{
    BaryWork W;
    W.partial = (uint32_t*)base;
    W.slot = W.partial + (size_t)batch * eval_blocks(n) * 8;
    W.sums = W.slot + (size_t)batch * 8;
    return W;
}
// "make inverses": d_inv[t * n + i] = 1 / (z_t - w^i) (one at i == m_t when z_t = w^(m_t)) for `points` points, point-major, by ONE launch and ONE
// batch_invert -- one host inversion and one synchronisation however many points.  d_tmp: points x n elements of workspace
int bary_inverses(uint64_t* d_inv, int log2n, int points, const host::Fr* z, const bool* on_domain, const size_t* m, uint64_t* d_tmp, Scratch& S,
                  hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    const uint32_t blocks = strided_blocks(n);
    const host::Fr root = host::fr_root_of_unity(log2n);
    BaryPoints P;
    for (int t = 0; t < BARY_MAX_POINTS; t++) {
        P.z_m256[t] = host::limbs_m256(z[t < points ? t : 0]);
        P.m[t] = (t < points && on_domain[t]) ? (uint32_t)m[t] : 0xffffffffu;
    }
    k_bary_denominators<<<dim3(blocks, (uint32_t)points), PT, 0, st>>>((uint32_t*)d_inv, (uint32_t)n, P, make_powtab(root),
                                                                       host::limbs_m261(host::fr_pow(root, (uint64_t)blocks * PT)));
    HIPCHK(launch_check());
    return batch_invert(d_inv, d_tmp, (size_t)points * n, S, st);
}
// "use inverses": evaluation and opening at one point over its n inverses; W: bary_work_bytes(n, batch) of workspace
static int bary_apply(const uint64_t* d_values, uint64_t* d_quotient, int log2n, size_t stride, int batch, const host::Fr& z, bool on_domain, size_t m,
                      const uint64_t* d_inverses, const BaryWork& W, host::Fr* h_out, Scratch& S, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    const uint32_t dblocks = eval_blocks(n), blocks = strided_blocks(n), mm = on_domain ? (uint32_t)m : 0xffffffffu;
    const uint32_t *v = (const uint32_t*)d_values, *d_inv = (const uint32_t*)d_inverses;
    uint32_t* q = (uint32_t*)d_quotient;
    if (!on_domain || q) {
        const host::Fr root = host::fr_root_of_unity(log2n);
        const PowTab T = make_powtab(root);
        const Limbs9 dstep = host::limbs_m261(host::fr_pow(root, (uint64_t)dblocks * PT));
        const dim3 dgrid(dblocks, (uint32_t)batch), qgrid(blocks, (uint32_t)batch);
        if (!on_domain) {
            k_bary_dot<<<dgrid, PT, 0, st>>>(v, stride, d_inv, (uint32_t)n, mm, T, host::limbs_m261(host::fr_from_u64(32)), dstep, W.partial);
            k_bary_finish<<<batch, PT, 0, st>>>(W.partial, dblocks, W.sums, host::limbs_m261(host::lagrange_open_scale(z, log2n)), W.slot, 1, 0);
            if (q) k_bary_quotient<<<qgrid, PT, 0, st>>>(v, q, stride, d_inv, W.slot, (uint32_t)n, mm);
        } else {
            HIPCHK(bary_stash(W.slot, d_values + 4 * m, stride, batch, st)); // before element m can be overwritten (q may be v)
            k_bary_quotient<<<qgrid, PT, 0, st>>>(v, q, stride, d_inv, W.slot, (uint32_t)n, mm);
            k_bary_dot<<<dgrid, PT, 0, st>>>(q, stride, d_inv, (uint32_t)n, mm, T, host::limbs_m261(host::fr_inv(host::fr_pow(root, (uint64_t)m))), dstep, W.partial);
            k_bary_finish<<<batch, PT, 0, st>>>(W.partial, dblocks, W.sums, host::limbs_m261(host::fr_neg(host::fr_one())), q, stride, mm);
        }
        HIPCHK(launch_check());
    } else {
        HIPCHK(bary_stash(W.slot, d_values + 4 * m, stride, batch, st));
    }
    return h_out ? bary_read_slots(W.slot, batch, h_out, S, st) : (int)BBGPU_OK;
}
int bary_open(const uint64_t* d_values, uint64_t* d_quotient, int log2n, size_t stride, int batch, const host::Fr& z, bool on_domain, size_t m,
              uint64_t* d_tmp, host::Fr* h_out, Scratch& S, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    int rc = ensure_pinned(S);
    if (rc) return rc;
    const size_t off_inv = (scan_scratch_bytes(n) + 64 + n * 32 + 64 + 63) & ~(size_t)63; // behind everything batch_invert asks for: its ensure() keeps the buffer
    const size_t off_work = off_inv + n * 32;
    rc = S.ensure(off_work + bary_work_bytes(n, batch));
    if (rc) return rc;
    uint64_t* d_inv = (uint64_t*)(S.base + off_inv);
    if (!on_domain || d_quotient) {
        rc = bary_inverses(d_inv, log2n, 1, &z, &on_domain, &m, d_tmp, S, st);
        if (rc) return rc;
    }
    return bary_apply(d_values, d_quotient, log2n, stride, batch, z, on_domain, m, d_inv, bary_work_at(S.base + off_work, n, batch), h_out, S, st);
}
// the same over inverses made earlier (an opening session, capi.hip): no denominators, no inversion; the workspace is the front of the scratch
int bary_open_with(const uint64_t* d_values, uint64_t* d_quotient, int log2n, size_t stride, int batch, const host::Fr& z, bool on_domain, size_t m,
                   const uint64_t* d_inverses, host::Fr* h_out, Scratch& S, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    int rc = ensure_pinned(S);
    if (rc) return rc;
    rc = S.ensure(bary_work_bytes(n, batch));
    if (rc) return rc;
    return bary_apply(d_values, d_quotient, log2n, stride, batch, z, on_domain, m, d_inverses, bary_work_at(S.base, n, batch), h_out, S, st);
}

static FoldCoeffs fold_coeffs(const host::Fr* gamma, int batch)
{
    FoldCoeffs G;
    for (int b = 0; b < FOLD_MAX_BATCH; b++) G.c[b] = host::limbs_m261(b < batch ? gamma[b] : host::fr_zero());
    return G;
}
// d_out[i] = (d_out[i] +) sum_b gamma_b v_{b,i}, canonical; any n
int fold(uint64_t* d_out, const uint64_t* d_values, size_t n, size_t stride, int batch, const host::Fr* gamma, bool accumulate, hipStream_t st)
{
    k_fold<<<pw_blocks(n), PT, 0, st>>>((uint32_t*)d_out, (const uint32_t*)d_values, stride, batch, fold_coeffs(gamma, batch), (uint32_t)n, accumulate ? 1u : 0u);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
// The opening of the fold F = sum_b gamma_b f_b at one point of a session: the values of (F(X) - F(z)) / (X - z) stored into d_quotient (n elements, not
// overlapping d_values) or added to it; h_out: null, or F(z).  The batch x n values are read ONCE:
//   off the domain   fold + dot in one trip (k_bary_fold_dot: F_i stored, F_i w^i inv_i summed), finish, quotient in place on F
//   on it            fold (k_fold), F_m -> slot by a copy, quotient in place (all but m), dot (q_i w^(i - m)), finish (* -1 -> q_m)
// When accumulating, F and its quotient live in the scratch and one more pass adds the n elements to d_quotient.
int bary_open_folded(const uint64_t* d_values, int log2n, size_t stride, int batch, const host::Fr* gamma, const host::Fr& z, bool on_domain, size_t m,
                     const uint64_t* d_inverses, uint64_t* d_quotient, bool accumulate, host::Fr* h_out, Scratch& S, hipStream_t st)
{
    const size_t n = (size_t)1 << log2n;
    const uint32_t dblocks = eval_blocks(n), blocks = strided_blocks(n), mm = on_domain ? (uint32_t)m : 0xffffffffu;
    int rc = ensure_pinned(S);
    if (rc) return rc;
    const size_t off_work = accumulate ? n * 32 : 0;
    rc = S.ensure(off_work + bary_work_bytes(n, 1));
    if (rc) return rc;
    const BaryWork W = bary_work_at(S.base + off_work, n, 1);
    uint32_t* F = accumulate ? (uint32_t*)S.base : (uint32_t*)d_quotient;
    const uint32_t *v = (const uint32_t*)d_values, *d_inv = (const uint32_t*)d_inverses;
    const host::Fr root = host::fr_root_of_unity(log2n);
    const PowTab T = make_powtab(root);
    const Limbs9 dstep = host::limbs_m261(host::fr_pow(root, (uint64_t)dblocks * PT));
    const FoldCoeffs G = fold_coeffs(gamma, batch);
    if (!on_domain) {
        k_bary_fold_dot<<<dblocks, PT, 0, st>>>(v, stride, batch, G, d_inv, (uint32_t)n, T, host::limbs_m261(host::fr_from_u64(32)), dstep, F, W.partial);
        k_bary_finish<<<1, PT, 0, st>>>(W.partial, dblocks, W.sums, host::limbs_m261(host::lagrange_open_scale(z, log2n)), W.slot, 1, 0);
        k_bary_quotient<<<blocks, PT, 0, st>>>(F, F, n, d_inv, W.slot, (uint32_t)n, mm);
    } else {
        k_fold<<<pw_blocks(n), PT, 0, st>>>(F, v, stride, batch, G, (uint32_t)n, 0u);
        HIPCHK(bary_stash(W.slot, (const uint64_t*)F + 4 * m, n, 1, st));
        k_bary_quotient<<<blocks, PT, 0, st>>>(F, F, n, d_inv, W.slot, (uint32_t)n, mm);
        k_bary_dot<<<dblocks, PT, 0, st>>>(F, n, d_inv, (uint32_t)n, mm, T, host::limbs_m261(host::fr_inv(host::fr_pow(root, (uint64_t)m))), dstep, W.partial);
        k_bary_finish<<<1, PT, 0, st>>>(W.partial, dblocks, W.sums, host::limbs_m261(host::fr_neg(host::fr_one())), F, n, mm);
    }
    HIPCHK(launch_check());
    if (accumulate) {
        rc = add_inplace_lanes(d_quotient, n, (const uint64_t*)F, n, n, 1, st);
        if (rc) return rc;
    }
    return h_out ? bary_read_slots(W.slot, 1, h_out, S, st) : (int)BBGPU_OK;
}

// ---- lane-batched forms: table plumbing ------------------------------------------------------------------------------------------------------------
int LaneTable::init(size_t bytes)
{
    if (d) return BBGPU_OK;
    HIPCHK(dev_malloc((void**)&d, bytes));
    if (hipHostMalloc((void**)&h, bytes) != hipSuccess) {
        (void)dev_free(d);
        d = h = nullptr;
        set_error("pinned lane table of %zu bytes refused", bytes);
        return BBGPU_ERR_HIP;
    }
    cap = bytes;
    used = flushed = 0;
    return BBGPU_OK;
}
void LaneTable::release()
{
    if (d) (void)dev_free(d);
    if (h) (void)hipHostFree(h);
    d = h = nullptr;
    cap = used = flushed = 0;
}
int LaneTable::reserve(size_t bytes, void** host, void** dev)
{
    const size_t at = (used + 63) & ~(size_t)63;
    if (!d || at + bytes > cap) {
        set_error("lane table full (%zu + %zu of %zu bytes)", at, bytes, cap);
        return BBGPU_ERR_SIZE;
    }
    *host = h + at;
    *dev = d + at;
    used = at + bytes;
    return BBGPU_OK;
}
int LaneTable::flush(hipStream_t st)
{
    if (used == flushed) return BBGPU_OK;
    HIPCHK(h2d_async(d + flushed, h + flushed, used - flushed, st));
    flushed = used;
    return BBGPU_OK;
}
// the records of one launch: copied into the pinned table, completed by `fill`, shipped
template <class T, class F> static int table_records(LaneTable& Tb, const T* A, int count, const T** dev, hipStream_t st, F fill)
{
    T* hrec = nullptr;
    if (int rc = Tb.push(count, &hrec, dev)) return rc;
    for (int l = 0; l < count; l++) {
        hrec[l] = A[l];
        fill(hrec[l], l);
    }
    return Tb.flush(st);
}

int z_terms_lanes(LaneTable& T, const ZTermsArgs* A, int lanes, const host::Fr& root, const host::Fr* beta, const host::Fr* gamma, hipStream_t st)
{
    const uint32_t blocks = strided_blocks(A[0].n);
    const PowTab rt = make_powtab(root);
    const Limbs9 step = host::limbs_m261(host::fr_pow(root, (uint64_t)blocks * PT));
    const ZTermsArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [&](ZTermsArgs& R, int l) {
            R.root = rt;
            R.step_m261 = step;
            z_terms_challenges(R, beta[l], gamma[l]);
        }))
        return rc;
    k_z_terms_lanes<<<dim3(blocks, lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int quotient_large_lanes(LaneTable& T, const QuotLargeArgs* A, int lanes, const host::Fr& root4n, const host::Fr* beta, const host::Fr* gamma, hipStream_t st)
{
    const uint32_t blocks = strided_blocks(A[0].n4);
    const PowTab rt = make_powtab(root4n);
    const Limbs9 step = host::limbs_m261(host::fr_pow(root4n, (uint64_t)blocks * PT)), g = host::limbs_m261(host::fr_from_limbs(FrHostP::GEN5));
    const QuotLargeArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [&](QuotLargeArgs& R, int l) {
            R.root = rt;
            R.g_m261 = g;
            R.step_m261 = step;
            quotient_large_challenges(R, beta[l], gamma[l]);
        }))
        return rc;
    k_quotient_large_lanes<<<dim3(blocks, lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int quotient_mid_lanes(LaneTable& T, const QuotMidArgs* A, int lanes, const host::Fr* alpha, const host::Fr* alpha_base, hipStream_t st)
{
    const QuotMidArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [&](QuotMidArgs& R, int l) { quotient_mid_challenges(R, alpha[l], alpha_base[l]); })) return rc;
    k_quotient_mid_lanes<<<dim3(pw_blocks(A[0].n2), lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int quotient_mimc_lanes(LaneTable& T, const QuotMimcArgs* A, int lanes, const host::Fr* alpha_base, const host::Fr* alpha_step, hipStream_t st)
{
    const QuotMimcArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [&](QuotMimcArgs& R, int l) {
            R.alpha_m261 = host::limbs_m261(alpha_step[l]);
            R.abase_fix_m261 = host::limbs_m261(host::fr_mul(alpha_base[l], host::fr_from_u64(32)));
        }))
        return rc;
    k_quotient_mimc_lanes<<<dim3(pw_blocks(A[0].n4), lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int quotient_bool_lanes(LaneTable& T, const QuotBoolArgs* A, int lanes, const host::Fr* c_left, const host::Fr* c_right, const host::Fr* c_out, hipStream_t st)
{
    const host::Fr f2 = host::fr_from_u64(32);
    const QuotBoolArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [&](QuotBoolArgs& R, int l) {
            R.cl_fix_m261 = host::limbs_m261(host::fr_mul(c_left[l], f2));
            R.cr_fix_m261 = host::limbs_m261(host::fr_mul(c_right[l], f2));
            R.co_fix_m261 = host::limbs_m261(host::fr_mul(c_out[l], f2));
        }))
        return rc;
    k_quotient_bool_lanes<<<dim3(pw_blocks(A[0].n2), lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int quotient_seq_lanes(LaneTable& T, const QuotSeqArgs* A, int lanes, const host::Fr* c, hipStream_t st)
{
    const QuotSeqArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st,
                               [&](QuotSeqArgs& R, int l) { R.c_fix_m261 = host::limbs_m261(host::fr_mul(c[l], host::fr_from_u64(32))); }))
        return rc;
    k_quotient_seq_lanes<<<dim3(pw_blocks(A[0].n2), lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int check_witness_lanes(LaneTable& T, const WitnessCheckArgs* A, int lanes, hipStream_t st)
{
    const Limbs9 one = host::limbs_m256(host::fr_one());
    const WitnessCheckArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [&](WitnessCheckArgs& R, int) { R.one_m256 = one; })) return rc;
    if (int rc = check_witness_preset(A[0].counts, A[0].first, lanes, st)) return rc;
    const dim3 grid(strided_blocks(A[0].n), lanes);
    k_check_gates_lanes<<<grid, PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    k_check_copies_lanes<<<grid, PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int expand_wires_lanes(LaneTable& T, const ExpandWiresArgs* A, int lanes, hipStream_t st)
{
    const ExpandWiresArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [](ExpandWiresArgs&, int) {})) return rc;
    k_expand_wires_lanes<<<dim3(pw_blocks((size_t)6 * A[0].n), lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int lincomb_lanes(LaneTable& T, const LinCombArgs* A, int lanes, const host::Fr* coeffs, hipStream_t st)
{
    const LinCombArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st, [&](LinCombArgs& R, int l) {
            for (int j = 0; j < R.count; j++) R.c[j] = host::limbs_m261(coeffs[(size_t)l * 12 + j]);
        }))
        return rc;
    k_lincomb_lanes<<<dim3(pw_blocks(A[0].n), lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int mul2c_lanes(LaneTable& T, const Mul2cArgs* A, int lanes, const host::Fr* c, hipStream_t st)
{
    const Mul2cArgs* dev = nullptr;
    if (int rc = table_records(T, A, lanes, &dev, st,
                               [&](Mul2cArgs& R, int l) { R.c_fix_m261 = host::limbs_m261(host::fr_mul(c[l], host::fr_from_u64(32))); }))
        return rc;
    k_mul2c_lanes<<<dim3(pw_blocks(A[0].n), lanes), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int sigma_prepare_lanes(LaneTable& T, const SigmaPrepArgs* A, int records, const host::Fr* gamma, hipStream_t st)
{
    const SigmaPrepArgs* dev = nullptr;
    if (int rc = table_records(T, A, records, &dev, st, [&](SigmaPrepArgs& R, int l) { R.gamma_m256 = host::limbs_m256(gamma[l]); })) return rc;
    k_sigma_prepare_lanes<<<dim3(pw_blocks(A[0].n_dst), records), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int copy_pad_lanes(LaneTable& T, const CopyPadArgs* A, int records, const host::Fr* c, hipStream_t st)
{
    const CopyPadArgs* dev = nullptr;
    if (int rc = table_records(T, A, records, &dev, st, [&](CopyPadArgs& R, int l) {
            R.scaled = c ? 1u : 0u;
            R.c_m261 = c ? host::limbs_m261(c[l]) : Limbs9{};
        }))
        return rc;
    k_copy_pad_lanes<<<dim3(pw_blocks(A[0].n_dst), records), PT, 0, st>>>(dev);
    HIPCHK(launch_check());
    return BBGPU_OK;
}
int add_inplace_lanes(uint64_t* d_a, size_t stride_a, const uint64_t* d_b, size_t stride_b, size_t n, int lanes, hipStream_t st)
{
    k_add_inplace_lanes<<<dim3(pw_blocks(n), lanes), PT, 0, st>>>((uint32_t*)d_a, stride_a, (const uint32_t*)d_b, stride_b, (uint32_t)n);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

int evaluate_lanes(const EvalJob* jobs, const int* zidx, int count, const host::Fr* z, int nz, LaneTable& T, Scratch& S, hipStream_t st)
{
    if (count < 1 || nz < 1) return BBGPU_ERR_ARG;
    if (int rc = S.ensure((size_t)count * 256 * 32 + 64)) return rc;
    EvalTabJob* J = nullptr;
    const EvalTabJob* dJ = nullptr;
    if (int rc = T.push(count, &J, &dJ)) return rc;
    std::vector<PowTab> tabs((size_t)nz);
    for (int k = 0; k < nz; k++) tabs[k] = make_powtab(z[k]);
    // z^(blocks * PT): the jobs of a proof have two lengths (n and 3n), so two values per point
    struct ZT { int zi; uint32_t blocks; Limbs9 v; };
    std::vector<ZT> zts;
    uint32_t maxb = 1;
    for (int j = 0; j < count; j++) {
        const size_t n = jobs[j].n;
        if (n == 0 || zidx[j] < 0 || zidx[j] >= nz) return BBGPU_ERR_ARG;
        const uint32_t blocks = eval_blocks(n);
        const Limbs9* zt = nullptr;
        for (const ZT& e : zts)
            if (e.zi == zidx[j] && e.blocks == blocks) zt = &e.v;
        if (!zt) {
            zts.push_back(ZT{ zidx[j], blocks, host::limbs_m261(host::fr_pow(z[zidx[j]], (uint64_t)blocks * PT)) });
            zt = &zts.back().v;
        }
        J[j].c = (const uint32_t*)jobs[j].coeffs;
        J[j].result = (uint32_t*)jobs[j].d_result;
        J[j].partial = (uint32_t*)S.base + (size_t)j * 256 * 8;
        J[j].n = (uint32_t)n;
        J[j].blocks = blocks;
        J[j].zT = *zt;
        J[j].T = tabs[zidx[j]];
        maxb = std::max(maxb, blocks);
    }
    if (int rc = T.flush(st)) return rc;
    k_eval_partial_tab<<<dim3(maxb, count), PT, 0, st>>>(dJ);
    k_sum_small_tab<<<count, PT, 0, st>>>(dJ);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace poly
} // namespace bbgpu
