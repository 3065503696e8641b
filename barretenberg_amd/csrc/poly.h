// poly.h -- internal interface of poly.hip (device-resident Fr polynomial helpers), used by plonk.hip and capi.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fe.hpp"
#include "host_fr.hpp"

namespace bbgpu {
namespace poly {

struct PowTab {
    Limbs9 p[24]; // base^(2^j), 2^261 form
};

// the points of one launch of k_bary_denominators (an opening session has up to BARY_MAX_POINTS; bary_open has one), by value
constexpr int BARY_MAX_POINTS = 4;
struct BaryPoints {
    Limbs9 z_m256[BARY_MAX_POINTS];
    uint32_t m[BARY_MAX_POINTS]; // the index of z on the domain, or >= n
};
// the multipliers of a fold (k_fold, k_bary_fold_dot), 2^261 form, by value
constexpr int FOLD_MAX_BATCH = 64;
struct FoldCoeffs {
    Limbs9 c[FOLD_MAX_BATCH];
};

// growable device workspace private to one stream of work (+ 4 KiB of pinned host memory for 32-byte read-backs)
struct Scratch {
    uint8_t* base = nullptr;
    size_t cap = 0;
    void* h_pinned = nullptr;
    int ensure(size_t bytes);
    void release();
};

struct ZTermsArgs {
    const uint32_t *w_l, *w_r, *w_o, *s1, *s2, *s3; // n Lagrange-form values each
    uint32_t *num, *den;
    uint32_t n;
    PowTab root;
    Limbs9 step_m261, beta_m256, beta_m261, beta_k1_m256, beta_k2_m256, gamma_m256;
};
struct QuotLargeArgs {
    const uint32_t *wl_f, *wr_f, *wo_f, *s1_f, *s2_f, *s3_f, *z_f; // 4n coset evaluations each
    uint32_t* q;
    uint32_t n4;
    PowTab root;
    Limbs9 g_m261, step_m261, beta_m256, beta_k1_m256, beta_k2_m256, gamma_m256;
};
struct QuotMidArgs {
    const uint32_t *z_f, *wl_f, *wr_f, *wo_f;           // 4n coset evaluations
    const uint32_t *l1;                                  // 2n
    const uint32_t *qm_f, *ql_f, *qr_f, *qo_f, *qc_f;    // 2n coset evaluations of the selectors, unscaled
    uint32_t* q;
    uint32_t n2;
    Limbs9 alpha_m256, alpha_fix_m261, alpha2_fix_m261, abase_m261, abase_fix2_m261, abase_fix3_m261;
};
struct QuotSeqArgs {
    const uint32_t* wo_f;   // 4n coset evaluations of w_o (read at index 2i + 4: the next gate's output wire)
    const uint32_t* qon_f;  // 2n coset evaluations of q_o_next, unscaled
    uint32_t* q;            // quotient_mid, accumulated into
    uint32_t n2;
    Limbs9 c_fix_m261;
};
struct QuotBoolArgs {
    const uint32_t *wl_f, *wr_f, *wo_f;    // 4n coset evaluations (read at index 2i)
    const uint32_t *qbl_f, *qbr_f, *qbo_f; // 2n coset evaluations of the bool selectors, unscaled
    uint32_t* q;                           // quotient_mid, accumulated into
    uint32_t n2;
    Limbs9 cl_fix_m261, cr_fix_m261, co_fix_m261; // alpha powers times 2^5
};
struct QuotMimcArgs {
    const uint32_t *wl_f, *wr_f, *wo_f; // 4n coset evaluations
    const uint32_t *qsel_f, *qcoef_f;   // 4n coset evaluations of q_mimc_selector / q_mimc_coefficient, unscaled
    uint32_t* q;                        // quotient_large, accumulated into
    uint32_t n4;
    Limbs9 alpha_m261, abase_fix_m261;  // alpha_step; alpha_base * 2^5
};
struct LinCombArgs {
    const uint32_t* p[12];
    Limbs9 c[12];
    const uint32_t* out_add; // optional addend (memory form), may be null
    uint32_t* out;
    uint32_t n;
    int count;
};

// ---- witness check (bbgpu_plonk_check_witness*, include/bbgpu.h: rows 0 .. n-2 only, the last row is not constrained) ----------------------------------------
// What the two check kernels leave per lane: 40 bytes, kept as two arrays (one per preset value) so that two memsets in front of the launches prepare every
// lane.  Integer atomics only, and none at all for a witness that satisfies the circuit.
struct WitnessCheckCounts {
    unsigned long long gate_failures, copy_failures; // preset 0
    uint32_t kinds, _pad;                            // OR of the kind masks of all failing rows
};
struct WitnessCheckFirst {          // preset all ones = none; atomicMin
    unsigned long long gate;        // (row << 32) | kind mask of that row
    unsigned long long copy;        // ((row << 2 | wire) << 32) | the position's mapping entry
};
struct WitnessCheckArgs {
    const uint32_t *w_l, *w_r, *w_o;                   // n Lagrange-form values each (any representative below 2^256)
    const uint32_t *q_m, *q_l, *q_r, *q_o, *q_c;       // selector VALUES
    const uint32_t* q_on;                              // sequential widget: q_o_next, else null
    const uint32_t *q_bl, *q_br, *q_bo;                // bool widget, else null
    const uint32_t *q_sel, *q_coef;                    // MiMC widget: q_mimc_selector, q_mimc_coefficient, else null
    const uint32_t *s1, *s2, *s3;                      // the three sigma mappings
    WitnessCheckCounts* counts;                        // this lane's record
    WitnessCheckFirst* first;
    uint32_t n;
    Limbs9 one_m256;
};
struct LaneTable;
// presets `lanes` consecutive records starting at A[0].counts / A[0].first, then the gate and the copy kernel: two launches however many lanes
int check_witness_lanes(LaneTable& T, const WitnessCheckArgs* A, int lanes, hipStream_t st);

// ---- wires from composer variables (bbgpu_plonk_prover_set_wire_map, the VARIABLES form of bbgpu_plonk_witness) ---------------------------------------------
// dst[k][i] = variables[index[k][i]], k = w_l, w_r, w_o: the loop of Composer::preprocess() (standard_composer.cpp:205-209) on the device, bit for bit.
// Every index is below num_variables: bbgpu_plonk_prover_set_wire_map refuses a map that is not, on the host, before it is uploaded.
struct ExpandWiresArgs {
    const uint32_t* variables;  // num_variables x 8 words, 16-byte aligned
    const uint32_t* index[3];   // n entries each
    uint32_t* dst[3];           // n x 8 words each
    uint32_t n, num_variables;
};
int expand_wires_lanes(LaneTable& T, const ExpandWiresArgs* A, int lanes, hipStream_t st); // one launch for the three wires of all lanes

struct EvalJob {
    const uint64_t* coeffs;
    size_t n;
    int zsel;           // evaluate at z[zsel]
    uint64_t* d_result; // 32-byte device slot
};
struct ScanJob {
    const uint64_t* in;
    uint64_t* out;      // may be null when only the total is wanted
    size_t n;
    bool reverse, inclusive;
    host::Fr z;         // Horner scans only
    uint64_t* d_total;  // optional 32-byte device slot, 16-byte aligned: the total is stored there by a kernel, not copied
};

// ---- the prover's round kernels (the lanes of plonk.hip: one for a single proof, up to 16 for a batch) ---------------------------------------------
// One launch serves every lane: blockIdx.y selects a RECORD of a device table -- one of the argument structs above (16 lanes of ZTermsArgs would not
// fit the kernel-argument space), holding the lane's vectors and its challenge-dependent constants.  The host writes the records
// into pinned memory and the table crosses with one copy in front of the launch; every workgroup reads one record, uniformly.
struct LaneTable {
    uint8_t *d = nullptr, *h = nullptr; // device table and its pinned mirror
    size_t cap = 0, used = 0, flushed = 0;
    int init(size_t bytes);
    void release();
    void reset() { used = flushed = 0; } // start of a batch: regions are never rewritten while a copy of them may be in flight
    int reserve(size_t bytes, void** host, void** dev);
    template <class T> int push(int count, T** host, const T** dev) { return reserve(sizeof(T) * (size_t)count, (void**)host, (void**)dev); }
    int flush(hipStream_t st); // everything pushed since the last flush, one copy
};
struct Mul2cArgs {
    uint32_t* out;
    const uint32_t *a, *b;
    uint32_t n;
    Limbs9 c_fix_m261;
};
struct SigmaPrepArgs {
    uint32_t* dst;
    const uint32_t *sigma, *w;
    uint32_t n, n_dst;
    Limbs9 gamma_m256;
};
struct CopyPadArgs { // dst[0..n_dst) = c * src[0..n_src) (or src itself, bit for bit: scaled = 0, the record of copy_pad), zeros behind
    uint32_t* dst;
    const uint32_t* src;
    uint32_t n_src, n_dst, scaled;
    Limbs9 c_m261;
};
struct EvalTabJob {
    const uint32_t* c;
    uint32_t *result, *partial; // 32-byte device slot; this job's 256 block partials
    uint32_t n, blocks;
    Limbs9 zT;
    PowTab T;
};
// `lanes` records each; A[l] carries lane l's vectors (and n), the functions fill in the constants
int z_terms_lanes(LaneTable& T, const ZTermsArgs* A, int lanes, const host::Fr& root, const host::Fr* beta, const host::Fr* gamma, hipStream_t st);
int quotient_large_lanes(LaneTable& T, const QuotLargeArgs* A, int lanes, const host::Fr& root4n, const host::Fr* beta, const host::Fr* gamma, hipStream_t st);
int quotient_mid_lanes(LaneTable& T, const QuotMidArgs* A, int lanes, const host::Fr* alpha, const host::Fr* alpha_base, hipStream_t st);
int quotient_mimc_lanes(LaneTable& T, const QuotMimcArgs* A, int lanes, const host::Fr* alpha_base, const host::Fr* alpha_step, hipStream_t st);
int quotient_bool_lanes(LaneTable& T, const QuotBoolArgs* A, int lanes, const host::Fr* c_left, const host::Fr* c_right, const host::Fr* c_out, hipStream_t st);
int quotient_seq_lanes(LaneTable& T, const QuotSeqArgs* A, int lanes, const host::Fr* c, hipStream_t st);
int lincomb_lanes(LaneTable& T, const LinCombArgs* A, int lanes, const host::Fr* coeffs /* lanes x 12 */, hipStream_t st);
int mul2c_lanes(LaneTable& T, const Mul2cArgs* A, int lanes, const host::Fr* c, hipStream_t st);
int sigma_prepare_lanes(LaneTable& T, const SigmaPrepArgs* A, int records, const host::Fr* gamma /* per record */, hipStream_t st);
int copy_pad_lanes(LaneTable& T, const CopyPadArgs* A, int records, const host::Fr* c /* per record; null: plain copy */, hipStream_t st);
// the same vector of every lane at base + lane * stride (elements), no per-lane constant
int add_inplace_lanes(uint64_t* d_a, size_t stride_a, const uint64_t* d_b, size_t stride_b, size_t n, int lanes, hipStream_t st);
int divide_by_pseudo_vanishing_lanes(uint64_t* d_coeffs, size_t stride, int lanes, int log2n, int log2N, hipStream_t st);
// `count` scans of one mode (0 = running products, 1 = Horner suffix sums) and one length (<= 2^22) in shared launches: the plan and the driver of
// product_scan / horner_suffix below, the phases launched from table records instead of by value.  jobs[j].d_total, where given, receives the total
// directly, in every form
int scan_lanes(int mode, const ScanJob* jobs, int count, LaneTable& T, Scratch& S, hipStream_t st);
// `count` evaluations, job j at z[zidx[j]]
int evaluate_lanes(const EvalJob* jobs, const int* zidx, int count, const host::Fr* z, int nz, LaneTable& T, Scratch& S, hipStream_t st);

PowTab make_powtab(const host::Fr& base);

int powers(uint64_t* d_out, size_t n, const host::Fr& base, const host::Fr& start, hipStream_t st);
int copy_pad(uint64_t* d_dst, const uint64_t* d_src, size_t n_src, size_t n_dst, hipStream_t st);
int mul_pointwise(uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n, hipStream_t st);

size_t scan_scratch_bytes(size_t n);
// exclusive / inclusive running products, prefix or suffix; d_out may be null when only the total is wanted
int product_scan(const uint64_t* d_in, uint64_t* d_out, size_t n, bool reverse, bool inclusive, Scratch& S, hipStream_t st, uint64_t* d_total);
// out_i = sum_{j >= i (inclusive) or j > i} in_j z^(j - i [- 1])
int horner_suffix(const uint64_t* d_in, uint64_t* d_out, size_t n, const host::Fr& z, bool inclusive, Scratch& S, hipStream_t st, uint64_t* d_total);
int evaluate_to_device(const uint64_t* d_coeffs, size_t n, const host::Fr& z, uint64_t* d_result, Scratch& S, hipStream_t st);
int evaluate(const uint64_t* d_coeffs, size_t n, const host::Fr& z, host::Fr* out, Scratch& S, hipStream_t st);
int batch_invert(uint64_t* d_v, uint64_t* d_tmp, size_t n, Scratch& S, hipStream_t st);

int sigma_from_mapping(uint64_t* d_out, const uint32_t* d_mapping, const uint64_t* d_roots, size_t n, hipStream_t st);
int divide_by_pseudo_vanishing(uint64_t* d_coeffs, int log2n, int log2N, hipStream_t st);
int lagrange_l1_fft(uint64_t* d_l1, uint64_t* d_tmp, int log2n, int log2N, Scratch& S, hipStream_t st);
// `batch` polynomials given by their values on the size-2^log2n domain (polynomial b at d_values + b * stride elements), evaluated at z (canonical) into
// h_out (may be null) and, with d_quotient (null, d_values itself or disjoint; same stride), opened there: the values of (f(X) - f(z)) / (X - z).
// on_domain / m: z == w^m, decided by the caller (host_lagrange_open.hpp).  d_tmp: n elements of workspace
int bary_open(const uint64_t* d_values, uint64_t* d_quotient, int log2n, size_t stride, int batch, const host::Fr& z, bool on_domain, size_t m,
              uint64_t* d_tmp, host::Fr* h_out, Scratch& S, hipStream_t st);
// Its two halves, for an opening session (capi.hip): the inverses 1 / (z_t - w^i) of up to BARY_MAX_POINTS points, point-major into d_inv (points x n
// elements; d_tmp: as many of workspace), by one launch and one batch_invert; then evaluation / opening at one point over ITS n inverses, as often as wanted
int bary_inverses(uint64_t* d_inv, int log2n, int points, const host::Fr* z, const bool* on_domain, const size_t* m, uint64_t* d_tmp, Scratch& S,
                  hipStream_t st);
int bary_open_with(const uint64_t* d_values, uint64_t* d_quotient, int log2n, size_t stride, int batch, const host::Fr& z, bool on_domain, size_t m,
                   const uint64_t* d_inverses, host::Fr* h_out, Scratch& S, hipStream_t st);
// the opening of F = sum_b gamma_b f_b over the same inverses: d_quotient (n elements, not overlapping d_values) is set or added to; h_out: null or F(z)
int bary_open_folded(const uint64_t* d_values, int log2n, size_t stride, int batch, const host::Fr* gamma, const host::Fr& z, bool on_domain, size_t m,
                     const uint64_t* d_inverses, uint64_t* d_quotient, bool accumulate, host::Fr* h_out, Scratch& S, hipStream_t st);
// d_out[i] = (d_out[i] +) sum_b gamma_b v_{b,i}: any n, batch <= FOLD_MAX_BATCH
int fold(uint64_t* d_out, const uint64_t* d_values, size_t n, size_t stride, int batch, const host::Fr* gamma, bool accumulate, hipStream_t st);

} // namespace poly
} // namespace bbgpu
