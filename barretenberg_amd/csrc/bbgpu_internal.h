// bbgpu_internal.h -- declarations shared by the HIP translation units and the C-ABI shim (capi.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <mutex>

#include "../../include/bbgpu.h"

namespace bbgpu {

void set_error(const char* fmt, ...);
// a failed HIP call: recorded with its place, and the calling function returns BBGPU_ERR_HIP
#define HIPCHK(x)                                                                                                      \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) {                                                                                        \
            set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));                                \
            return BBGPU_ERR_HIP;                                                                                      \
        }                                                                                                              \
    } while (0)

// capi.hip: EVERY device allocation, host<->device copy of a caller's buffer and launch check of the library goes through these four, so that
// (i) a test can make the k-th one fail on a machine that HAS a GPU (BBGPU_FAIL_AT / bbgpu_fault_inject: "alloc:k", "h2d:k", "d2h:k", "launch:k" -- the
// error contract of the drop-in boundary, SURVEY 8b "Errors"; no kernel reads any of this) and (ii) the live device allocations are counted
// (bbgpu_fault_stats: a leak on an error path shows as allocations that outlive bbgpu_shutdown()).
hipError_t dev_malloc(void** p, size_t bytes);
hipError_t dev_free(void* p);
hipError_t h2d_async(void* dst, const void* src, size_t bytes, hipStream_t st);
hipError_t d2h_async(void* dst, const void* src, size_t bytes, hipStream_t st);
hipError_t launch_check(); // hipGetLastError() after a launch (or a chain of launches)
// a device buffer that is freed on every way out of a function unless it was handed on (release())
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)dev_free(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    template <class T> T* release() { T* r = static_cast<T*>(p); p = nullptr; return r; }
};
// the N events between the timed stages of a call (bbgpu_set_timing): made only when timing is on, destroyed on every way out of the function
template <int N> struct StageEvents {
    hipEvent_t e[N] = {};
    bool on = false;
    StageEvents() = default;
    StageEvents(const StageEvents&) = delete;
    StageEvents& operator=(const StageEvents&) = delete;
    ~StageEvents()
    {
        for (hipEvent_t v : e)
            if (v) (void)hipEventDestroy(v);
    }
    int create(bool timed)
    {
        on = timed;
        if (on)
            for (hipEvent_t& v : e) HIPCHK(hipEventCreate(&v));
        return BBGPU_OK;
    }
    int mark(int k, hipStream_t st) // nothing when timing is off
    {
        if (on) HIPCHK(hipEventRecord(e[k], st));
        return BBGPU_OK;
    }
    int ms(int a, int b, float* out) // from mark a to mark b, both complete; timing is on
    {
        HIPCHK(hipEventElapsedTime(out, e[a], e[b]));
        return BBGPU_OK;
    }
};
void fault_absorbed();     // a failure the library rode out by itself (an SRS kept without its window tables): counted, so a test can tell it from a lost injection

// ntt.hip
int ntt_device(uint64_t* d_coeffs, uint64_t* d_scratch, int log2n, int kind, const uint64_t* constant_m256, hipStream_t st);
int ntt_device_batch(uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* d_scratch, int log2n, int kind, const uint64_t* constant_m256,
                     hipStream_t st);
void ntt_release_tables();
size_t ntt_table_bytes(size_t* cap_out, int* sets_out); // device bytes the cached twiddle / twist tables hold now, their budget, how many domain sizes

// msm.hip
namespace host { struct Xyzz; }
struct MsmTiming {
    int count = 0;
    float ms[8]; // [0] total device time, then digits, sort, accumulate kernel, merge, row/col folds, slices+collect,
                 // [7] accumulate kernel without the time it sat queued behind the previous MSM's accumulation (two MSMs in flight)
};
struct MsmWorkspace {
    uint8_t* base = nullptr;
    size_t cap = 0;
    void* h_out = nullptr; // pinned
    static size_t bytes_needed(size_t n, int c, int nw, int ng = 0); // nw (job, window) pairs, ng bucket sets (0: one per pair = no window tables)
    int ensure(size_t bytes);
    void release();
};
// One MSM of a slot may be issued as several PIECES -- point ranges against different segments of the window tables (an SRS above 2^20 points keeps
// one table per <= 2^20-point segment, capi.hip), enqueued back to back on the slot's stream and sharing its workspace in stream order; every piece
// writes its own 64-slot groups of the pinned result array and the host adds the piece sums (a sum over a range of points is a plain term of the MSM).
struct MsmPiece {
    uint32_t c = 0, nw = 0, wb = 0, hbits = 0, lbits = 0;
    uint32_t hout_group = 0; // first 64-slot group of this piece in ws.h_out
    bool trivial = false;
};
// "accumulation ended" events of the last SIZE timed MSMs of one device context, in issue order (msm.hip acc_ring_record / finish_timing).  One ring
// per context, shared by its slots: the contexts of bbgpu_init_devices issue concurrently, and may sit on different devices.
struct AccRing {
    static constexpr int SIZE = 8;
    hipEvent_t end[SIZE] = {};
    uint64_t seq = 0; // number of timed accumulations issued so far
    void release();
};
constexpr int MSM_MAX_JOBS = 4;        // MSMs over the same points issued as one batch (one bucket set each)
constexpr int MSM_MAX_PIECES = 64;      // per slot: an MSM without a free helper slot keeps all its pieces on one
constexpr uint32_t MSM_HOUT_GROUPS = 256; // 64-slot groups of the pinned result array (pieces x jobs, or the windows of one table-less piece): 2 MiB per slot
struct MsmSlot {
    MsmWorkspace ws;
    MsmPiece piece[MSM_MAX_PIECES];
    int npieces = 0;
    bool append = false; // set by the caller before an issue: add a piece to the MSM already issued on this slot instead of starting a new one
    int helper = -1;     // capi.hip: a second slot (own stream and workspace) that carries every other piece of this ticket, or -1
    bool is_helper = false; // this slot is pending as the helper of another ticket: collected through its owner only
    bool reserved = false;  // capi.hip: a synchronous entry point is cycling its jobs / ranges through this slot: not to be taken as a helper meanwhile
    hipStream_t stream = nullptr; // the slot's own stream (used when the caller passes none)
    hipEvent_t done = nullptr;
    hipEvent_t ev[8] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    bool pending = false, trivial = false, timed = false, timed_light = false;
    size_t n = 0;
    uint32_t jobs = 1;
    uint64_t acc_seq = 0; // position of this MSM's accumulation in its context's sequence of timed accumulations (0 = none)
    AccRing* acc_ring = nullptr; // capi.hip: the ring of the slot's context (null: no timed accumulation is recorded)
    // set by the caller before an issue: other MSMs are in flight, so this one is paced by the instructions it issues, not by its dependent chain
    // (msm_issue_batch then takes longer chunks and the two-step row / column sums)
    bool throughput = false;
    void release();
};
int msm_choose_c(size_t n);
int msm_num_windows(int c);
int msm_issue_batch(MsmSlot& S, const uint32_t* d_srs, const uint32_t* d_tab, size_t tab_stride, int tab_c, const uint64_t* const* d_scalars_v, int jobs,
                    size_t n, int wb, int we, hipStream_t st, int want_timing, uint32_t row_i0 = 0, uint32_t row_i1 = 0xffffffffu, uint32_t brow0 = 0,
                    uint32_t brow1 = 0xffffffffu);
int msm_issue_buckets(MsmSlot& S, const uint32_t* d_srs, const uint32_t* d_tab, size_t tab_stride, int tab_c, const uint64_t* d_scalars, size_t n,
                      uint32_t share, uint32_t share_count, hipStream_t st, int want_timing);
int msm_issue_rows(MsmSlot& S, const uint32_t* d_srs, const uint32_t* d_tab, size_t tab_stride, int tab_c, const uint64_t* d_scalars, size_t n,
                   uint64_t row_begin, uint64_t row_end, hipStream_t st, int want_timing);
int msm_finish_batch(MsmSlot& S, host::Xyzz* results, MsmTiming* timing);
int srs_build_table(const uint32_t* d_srs, size_t n, int c, int num_windows, int w_begin, int w_end, uint32_t** d_alloc_out, uint32_t** d_tab_out, hipStream_t st);
int srs_upload(const uint64_t* host_table, size_t n, uint32_t** d_srs_out, hipStream_t st, size_t stride_bytes = 128);
int srs_upload_into(const uint64_t* host_table, size_t n, uint32_t* d_raw, uint32_t* d_srs, hipStream_t st, size_t stride_bytes);
int srs_generate(const uint64_t* x_mont256, size_t first, size_t n, uint32_t** d_srs_out, uint64_t* host_table_out, hipStream_t st);
int srs_export(const uint32_t* d_srs, size_t n, uint32_t* d_table, hipStream_t st);

// srs_update.hip: rows times powers of y into a new allocation (bbgpu_srs_update)
int srs_update_rows(const uint32_t* d_in, size_t n, uint64_t first_power, const uint64_t* y_mont256, uint32_t** d_out_rows, uint64_t* host_table_out, hipStream_t st,
                    float* kernel_ms = nullptr);

// srs_check.hip: the O(n) device parts of bbgpu_srs_check that are not an MSM
struct SrsCurveFindings {
    unsigned long long bad_points, first_bad_point; // rows with y^2 != x^3 + 3, the smallest of them (the caller starts it at ~0)
    uint32_t first_is_generator, _pad;
};
int srs_check_curve(const uint32_t* d_srs, size_t n, const uint64_t generator_m261[8], SrsCurveFindings* d_out, hipStream_t st);
int srs_check_scalars(const uint64_t seed[4], size_t count, uint64_t* d_out, hipStream_t st);

// srs_lagrange.hip: rows [0, n) of a resident table in the Lagrange basis of the size-n domain, into a new allocation (bbgpu_srs_lagrange)
int srs_lagrange_rows(const uint32_t* d_in, size_t n, int log2n, const uint32_t winv_m261[9], const uint64_t ninv_plain[4], SrsCurveFindings* d_find,
                      SrsCurveFindings* found, uint32_t** d_out_rows, uint64_t* host_table_out, hipStream_t st, float* ms3 = nullptr);

// kzg_open_cosets.hip: the proofs of a polynomial on every coset of its domain (bbgpu_kzg_open_cosets_setup(_bounded), bbgpu_kzg_open_cosets_device); d =
// 2^log2d is the degree bound of the setup, n without one.  bbgpu_kzg_open_all_setup and bbgpu_kzg_open_all_device are log2l = 0, log2d = log2n
int kzg_open_cosets_string(const uint32_t* d_in, int log2d, int log2l, const uint32_t W_m261[9], uint32_t** d_S, hipStream_t st);
int kzg_open_cosets_t(const uint64_t* d_coeffs, size_t stride_elems, int batch, int log2d, int log2l, uint64_t* d_t, hipStream_t st);
int kzg_open_cosets_chain(const uint32_t* d_S, uint64_t* d_that, uint32_t* d_scratch, int log2n, int log2l, int log2d, int batch, const uint32_t c32[9],
                          const uint32_t Winv[9], const uint32_t psi[9], hipStream_t st, float* ms4 = nullptr);

// plonk_verify.hip: the device parts of a verify call (bbgpu_plonk_verify_batch, bbgpu_plonk_verify_multi) that are not an MSM
struct VerifyDeviceBuffers {
    const uint64_t* proofs; // count x BBGPU_PLONK_PROOF_WORDS
    uint32_t *rows_own, *rows_other; // count x 9 and count x 2 resident rows (64 bytes)
    uint64_t *scal_own, *scal_other; // the scalars on them, 4 words each
    uint64_t* shared;                // [shared point][proof] x 4 words: rho_j s_jk
    uint32_t* status;                // count
};
// What the kernels read about one circuit: a verifier handle keeps it, a call of one circuit passes it as a kernel argument, a call of several lays
// them out as a table on the device.  192 bytes (a multiple of 64: the table sits in the staging buffer before the shared rows); the three constants 12
// words apart, each read from the table by three 16-byte loads
struct VerifyRecord {
    uint32_t log2n, widgets, num_vk;
    uint32_t base;      // the circuit's first shared row among the rows (and scalars) of A: set per call
    uint32_t skip_mask; // key points at infinity: their scalars are written as zero
    uint32_t pad[7];
    uint32_t root[12], root_inv[12], n_inv[12]; // omega, omega^-1, 1 / n: Montgomery-261, 29-bit limbs (host_fr.hpp limbs_m261) in the first nine words
};
static_assert(sizeof(VerifyRecord) == 192, "VerifyRecord: 192 bytes");
// the circuits of one call: the one record (host memory), or, with `one` null, the device table, proof j's index into it at d_circuit[j], and the
// largest num_vk + 1 among the records
struct VerifyCircuits {
    const VerifyRecord* one = nullptr;
    const VerifyRecord* d_records = nullptr;
    const uint32_t* d_circuit = nullptr;
    int num_circuits = 1, max_shared = 0;
};
int plonk_verify_terms(const VerifyCircuits& C, const uint64_t seed[4], size_t count, const VerifyDeviceBuffers& B, hipStream_t st);
int plonk_verify_fold(const VerifyCircuits& C, const uint64_t* d_shared, size_t count, size_t m, uint64_t* d_out, hipStream_t st); // the first m proofs

// kzg_check.hip: the device parts of a check of KZG openings (bbgpu_kzg_check_openings, bbgpu_kzg_check_open_all) that are not an MSM
struct KzgFindings {
    unsigned long long bad_points, first_key; // finite points off the curve; the smallest 2 t + (1 for the proof) among them (the caller starts it at ~0)
};
struct KzgCheckBuffers {
    const uint64_t *proofs, *commitments, *z, *y; // the caller's arrays on the device: count x 8, count x 8 (per-claim layout), count x 4 (not open-all), count x 4
    const uint32_t* which;                        // count labels (shared layout with explicit labels)
    uint32_t* rows;                               // the claims' resident rows: (C_t, pi_t) in the per-claim layout, else pi_t
    uint64_t *scal_a, *scal_b;                    // the scalars of A and of B on those rows
    uint64_t *term_y, *term_rho;                  // count x 4 words each: rho_t y_t; rho_t (shared layouts)
    uint64_t* partial;                            // (S + 1) x KZG_FOLD_MAX_RANGES x 4 words
    KzgFindings* find;
};
constexpr size_t KZG_FOLD_RANGE = 4096;      // claims per workgroup of the fold until KZG_FOLD_MAX_RANGES ranges are in use
constexpr size_t KZG_FOLD_MAX_RANGES = 256;  // one thread of the finish kernel per range
uint32_t kzg_check_claim_threads(size_t count); // threads of the k_kzg_claims grid: the stride of the open-all form's powers
uint32_t kzg_check_fold_ranges(size_t m);
int kzg_check_claims(const KzgCheckBuffers& B, const uint64_t seed[4], size_t count, bool per_claim, bool open_all, int log2n, const uint32_t omega_m261[9],
                     const uint32_t step_m261[9], hipStream_t st);
int kzg_check_fold(const KzgCheckBuffers& B, size_t m, size_t S, int log2n, uint64_t skip_mask, uint64_t* d_out, hipStream_t st); // the first m claims

// kzg_check_cells.hip: the device parts of a check of KZG cell proofs (bbgpu_kzg_check_cells, bbgpu_kzg_check_open_cosets) that are not an MSM.
// l = 2^log2l values per cell, m = 2^(log2n - log2l) cells per polynomial.  Labelled form: which / cell given, the values of cell t at values[t l ..].
// Open-cosets form (which == cell == null): cell t = b m + k, its values at values[b n + k + m j], j < l.
struct KzgCellsBuffers {
    const uint64_t *proofs, *values; // the caller's arrays on the device: count x 8 words; count x l x 4 words, or batch x n x 4
    const uint32_t *which, *cell;    // count labels and cell indices (labelled form)
    uint32_t* rows;                  // the cells' rows pi_t: 64 bytes each, Montgomery-261, canonical
    uint64_t *scal_a, *scal_b;       // the scalars of A and of B on those rows: rho_t psi^(k_t), rho_t
    uint64_t *term_rho, *term;       // count x 4 words: rho_t; count x l x 4 words: T_{t,i} = rho_t a_{t,i}
    uint64_t* partial;               // (S + l) x KZG_FOLD_MAX_RANGES x 4 words
    const uint32_t* roots;           // KZG_CELLS_MAX_COSET x 9 limbs: zeta^(-e), Montgomery-261 (the first l are read)
    KzgFindings* find;
};
constexpr int KZG_CELLS_MAX_COSET = 64;
constexpr uint32_t KZG_CELLS_COEF_MAX_BLOCKS = 1024; // workgroups of the coefficient kernel; the rest by its stride
int kzg_cells_claims(const KzgCellsBuffers& B, const uint64_t seed[4], size_t count, int log2n, int log2l, const uint32_t psi_m261[9], hipStream_t st);
// omega_inv: omega^-1; into: 2^5 / l -- what takes a value from memory form to Montgomery-261 and divides by l in one product
int kzg_cells_coefficients(const KzgCellsBuffers& B, size_t count, int log2n, int log2l, const uint32_t omega_inv_m261[9], const uint32_t into_m261[9],
                           hipStream_t st, float* ms = nullptr);
// the scalars of the head of A over the cells [0, cells): d_out[c] for the S shared commitments, d_out[S + i] = -s_i on P_i
int kzg_cells_fold(const KzgCellsBuffers& B, size_t cells, size_t S, int log2n, int log2l, uint64_t skip_mask, uint64_t* d_out, hipStream_t st);
// The layout entries (bbgpu_kzg_check_cells_layout, bbgpu_kzg_check_open_cosets_layout): S <= 2^16 commitments tested and converted on the device, the
// cells grouped by label once per call, the S commitment scalars by a fold over the lists.  which == null: the open-cosets form, label c is the cells
// [c m, (c + 1) m) and nothing is grouped (cnt / off / poff / perm are not read).
struct KzgLayoutBuffers {
    const uint64_t* commitments; // S x 8 words as the caller gave them
    const uint32_t* which;       // the count labels on the device (labelled form)
    uint32_t* rows;              // the S rows of the commitments in the table of A
    uint64_t* skip;              // ceil(S / 64) words: bit c set for a commitment at infinity
    KzgFindings* find;           // bad_points: finite commitments off the curve; first_key: the smallest index among them
    uint32_t *cnt, *off, *poff;  // S counters; S + 1 starts of the lists in perm; S + 1 first pieces
    uint32_t* perm;              // the count cells, label by label
    uint64_t* partial;           // kzg_layout_max_pieces x 4 words
};
constexpr size_t KZG_LAYOUT_PIECE = 1024; // cells per wave of the list fold: 16 per lane, the chain k_kzg_cells_fold runs over a range of KZG_FOLD_RANGE
static_assert(KZG_LAYOUT_PIECE <= KZG_FOLD_RANGE && KZG_LAYOUT_PIECE % 64 == 0, "a piece is at most a range and whole waves");
size_t kzg_layout_max_pieces(size_t count, size_t S, int log2m, bool cosets);
int kzg_layout_group(const KzgLayoutBuffers& L, size_t count, size_t S, hipStream_t st, float* ms = nullptr);
int kzg_layout_fold(const KzgLayoutBuffers& L, const uint64_t* d_term_rho, size_t cells, size_t count, size_t S, int log2m, uint64_t* d_out, hipStream_t st,
                    float* ms = nullptr);

// kzg_recover_cells.hip: the device parts of bbgpu_kzg_recover_cells that are neither a transform nor the batch inversion.  l = 2^log2l values per cell,
// m = 2^(log2n - log2l) cells per polynomial, mu of them missing (d_missing: ascending; may be null when mu == 0).
struct RecoverFindings {
    unsigned long long first_bad, first_bug; // the smallest nonzero coefficient in [d, count l) and in [count l, n) (the caller starts both at ~0)
};
constexpr int KZG_RECOVER_TILE = 256;                  // roots of missing cells per LDS tile of k_recover_vanish
constexpr uint32_t KZG_RECOVER_TAIL_MAX_BLOCKS = 1024; // workgroups per polynomial of the tail kernel; the rest by its stride
int kzg_recover_group_log2(int log2m); // log2 of the lanes that share one a in k_recover_vanish
// d_z[a] = z_a as a Montgomery-261 multiplier, d_zc[a] = z'_a x 2^-5 in the memory format (its inverse there is the multiplier 1 / z'_a): m x 4 words each
// d_roots: 9 x mu words of workspace for psi^k, k missing
int kzg_recover_vanish(const uint32_t* d_missing, size_t mu, int log2n, int log2l, uint32_t* d_roots, uint64_t* d_z, uint64_t* d_zc, hipStream_t st);
// The back end of bbgpu_kzg_recover_cells AND bbgpu_kzg_recover_cells_each.  Polynomial b has d_off[b + 1] - d_off[b] cells, their values from element
// d_off[b] l of d_values on, their indices from d_cell[d_off[b] & cell_mask] on; it misses the d_mu[b] cells at d_missing[b missing_stride ..]; its z and
// z' lie b z_stride elements into theirs.  Each entry: cell_mask = ~0, missing_stride = M (below), z_stride = m.  Same-set entry: d_off[b] = b count,
// d_mu[b] = mu, and mask and strides 0 -- one row of each for all.
struct RecoverLists {
    const uint32_t *d_off, *d_mu, *d_cell, *d_missing;
    uint32_t cell_mask, missing_stride, z_stride;
};
int kzg_recover_scatter(const uint64_t* d_values, const RecoverLists& L, const uint64_t* d_z, int log2n, int log2l, int batch, uint64_t* d_out, size_t stride_elems,
                        hipStream_t st);
int kzg_recover_divide(uint64_t* d_q, size_t stride_elems, int batch, const uint64_t* d_inv, const RecoverLists& L, int log2n, int log2l, hipStream_t st);
int kzg_recover_tail(uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* d_copy, int log2n, int log2l, size_t degree_bound, const RecoverLists& L,
                     RecoverFindings* d_find, hipStream_t st);

// kzg_recover_each.hip: the device parts of bbgpu_kzg_recover_cells_each that are neither a transform nor the batch inversion.  Polynomial b lists the
// cells d_cell[d_off[b] .. d_off[b + 1]) and misses d_mu[b]; row b of d_missing (M entries, M the common power of two >= every mu_b, >= 1) holds its
// missing cells and then ~0.  The product tree lives in batch x 2 M elements: at the level of nodes of degree D every node has a slot of 2 D elements,
// its D low coefficients (the leading 1 is implied) and D zeros.
// T: roots per leaf of the product tree, T / 64 waves of k_each_leaves.  128 and 256 compile too (a leaf then spans waves that exchange through LDS): the
// comparison of profiles/kzg_recover_each.txt is a build with 256 here; BbGpu.RECOVER_EACH_LEAF (bbgpu.py) mirrors the value
constexpr int KZG_RECOVER_EACH_LEAF = 64;
constexpr size_t kzg_recover_each_table_words(int log2m) { return (((size_t)1 << ((log2m + 1) / 2)) + ((size_t)1 << (log2m / 2))) * 9; } // k_each_powers
int kzg_recover_each_leaves(const uint32_t* d_missing, int batch, size_t M, int log2m, uint64_t* d_tree, hipStream_t st);
int kzg_recover_each_pair(uint64_t* d_tree, size_t pairs, int log2s, hipStream_t st);
int kzg_recover_each_gather(const uint64_t* d_tree, const uint32_t* d_mu, int batch, size_t M, int log2n, int log2l, uint32_t* d_tab, uint64_t* d_zin,
                            uint64_t* d_zcin, hipStream_t st);

// g1_recover.hip: the device parts of bbgpu_g1_ntt and bbgpu_g1_recover.  Columns of n = 2^log2n scratch points (128 bytes each), column b at slot b n;
// batch x n <= 2^20.  Nothing here synchronises.  The last argument of load, scale, scalars and verdict is what bbgpu_g1_recover_each adds -- every column
// with its own rows --; its default is the same-set form.  d_off: the batch + 1 row offsets: column b's points start at point d_off[b] of d_in, d_slot_of and
// d_tab hold batch x n entries, and the verdict takes count_b = d_off[b + 1] - d_off[b].  per_column: d_tab holds batch x n entries.  cols: z, z' and the
// tables kz, kq hold cols x n entries (0: n).
int g1_cols_load(const uint32_t* d_in, size_t count, const uint32_t* d_slot_of, const uint64_t* d_tab, const uint64_t* k_plain, uint32_t* d_scratch, int log2n,
                 int batch, hipStream_t st, const uint32_t* d_off = nullptr);
int g1_cols_transform(uint32_t* d_scratch, int log2n, int batch, const uint32_t root_m261[9], hipStream_t st);
int g1_cols_transform_rows(uint32_t* d_scratch, int log2n, int batch, const uint32_t root_m261[9], hipStream_t st); // the bench's comparison only
int g1_cols_scale(const uint32_t* d_src, uint32_t* d_dst, const uint64_t* d_tab, int log2n, int batch, hipStream_t st, bool per_column = false);
int g1_cols_scalars(const uint64_t* d_z, const uint64_t* d_zci, uint64_t* d_tabs, int log2n, const uint32_t ninv_plain[9], const uint32_t g_m261[9],
                    const uint32_t ginv_m261[9], hipStream_t st, int cols = 0);
int g1_cols_verdict(const uint32_t* d_scratch, int log2n, int batch, size_t degree_bound, size_t present, RecoverFindings* d_find, hipStream_t st,
                    const uint32_t* d_off = nullptr);
int g1_cols_finish(const uint32_t* d_scratch, uint32_t* d_out, int log2n, int batch, hipStream_t st);
// z and z' x 2^-5 of EVERY column, batch x n x 4 words each, in the forms of kzg_recover_vanish.  d_moff: batch + 1 offsets into d_missing, column b's
// missing rows ascending at d_missing[d_moff[b] .. d_moff[b + 1]), fewer than n of them; d_roots: n x 9 words of workspace
int g1_cols_vanish(const uint32_t* d_moff, const uint32_t* d_missing, int log2n, int batch, uint32_t* d_roots, uint64_t* d_z, uint64_t* d_zc, hipStream_t st);

// fr_columns.hip: the device parts of bbgpu_fr_ntt_columns_device and bbgpu_fr_recover_columns_device.  A resident row-major matrix of rows = 2^log2rows
// rows (<= 2^11), row r at element r stride_elems; a codeword is a column.  Nothing here synchronises.  d_tabs: fr_cols_table_words(log2rows, entries)
// words, entries = sets x rows for the decoder (d_z, d_zci: z as a Montgomery-261 multiplier and the batch inversion of z' x 2^-5, the forms of
// g1_cols_vanish, `entries` elements each) and 0 for the transform (d_z, d_zci not read).  d_moff: the sets + 1 offsets of g1_cols_vanish; d_present: bit
// s rows + i set where set s lists row i; d_bad: null, or width words that receive every column's smallest index in [d, count_s), ~0 for none; d_find: two
// words the caller starts at ~0: the smallest (column << 32 | index) in [d, count_s) and in [count_s, rows).
size_t fr_cols_table_words(int log2rows, size_t entries);
int fr_cols_tables(const uint64_t* d_z, const uint64_t* d_zci, size_t entries, int log2rows, uint32_t* d_tabs, hipStream_t st);
int fr_cols_transform(uint64_t* d_rows, size_t width, size_t stride_elems, int log2rows, bool inverse, const uint32_t* d_tabs, hipStream_t st);
int fr_cols_decode(uint64_t* d_rows, size_t width, size_t stride_elems, int log2rows, int sets, size_t degree_bound, const uint32_t* d_tabs,
                   const uint32_t* d_moff, const uint32_t* d_present, uint32_t* d_bad, unsigned long long* d_find, hipStream_t st);

// capi.hip: the caller's host buffers cross the link through the library's OWN pinned buffers (see host_to_device)
int host_to_device(void* d_dst, const void* h_src, size_t bytes, hipStream_t st);
int device_to_host_sync(void* h_dst, const void* d_src, size_t bytes, hipStream_t st, bool* touched = nullptr); // *touched: h_dst may have been written (even on failure)
void host_stage_release();
int bind_calling_thread(); // initialises the library if need be and makes the bound device the calling thread's current one (HIP's current device is per thread)

// plonk.hip
std::mutex& plonk_mutex();        // taken BEFORE capi.hip's mutex wherever both are held
void plonk_release_all_locked();  // caller holds plonk_mutex()
uint64_t plonk_lane_bytes();      // device bytes the batch lanes of all provers hold (lock-free: read by bbgpu_memory_stats under capi.hip's mutex)

} // namespace bbgpu
