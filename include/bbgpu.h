/*
 * bbgpu.h -- C ABI of libbbgpu.so: MI355X (gfx950) implementations of barretenberg's PLONK-prover hot path,
 * BN254 G1 Pippenger MSM and radix-2 NTT / coset-FFT over Fr.
 *
 * Every entry point names the reference interface it replaces (paths under /root/reference/src/barretenberg/).
 * Conventions are the reference's own:
 *   field element   = 4 x uint64_t little-endian limbs, Montgomery form (x * 2^256 mod p)      fields/field.hpp:19-22
 *   affine G1 point = {x, y} = 8 x uint64_t; Jacobian = {x, y, z} = 12 x uint64_t               groups/group.hpp:17-28
 *   point at infinity <=> bit 63 of y limb 3                                                    groups/group.hpp:133-151
 *   scalars may be any representative in [0, 2r); NTT inputs in [0, 2^256); NTT outputs canonical [0, r)
 *   MSM results are returned NORMALISED: z = fq::one, x,y canonical (what batched_scalar_multiplications hands the
 *   prover, scalar_multiplication.cpp:765; any Jacobian representative is legal for pippenger(), :457-476)
 * All functions return BBGPU_OK (0) or a negative error code; bbgpu_last_error() describes the last failure of the
 * calling thread.  The GPU entry points have NO CPU fallback: if no GPU / no code object / no memory, they fail loudly.  The reference's
 * C++ signatures cannot report an error, so the C++ shim -- and only it -- answers a failed call with the bbgpu_host_* entries at the
 * end of this header (SURVEY 8b "the C++ shim must turn non-zero into CPU fallback"); BBGPU_SHIM_STRICT=1 makes it abort instead.
 */
#ifndef BBGPU_H
#define BBGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    BBGPU_OK = 0,
    BBGPU_ERR_HIP = -1,   /* a HIP runtime call failed (no device, out of memory, launch failure) */
    BBGPU_ERR_SIZE = -2,  /* size not supported (NTT: n must be 2^k, 2 <= n <= 2^28 = the two-adicity of the field) */
    BBGPU_ERR_ARG = -3,   /* null pointer / bad enum / unknown handle */
    BBGPU_ERR_STATE = -4, /* library not initialised / every MSM slot in flight / a table that lacks what the call needs */
    BBGPU_ERR_LOST = -5,  /* an IN-PLACE host-buffer call failed while its result was being copied back: the caller's buffer may hold a mixture of
                             input and output (the one failure the shim cannot answer with a host computation) */
    BBGPU_ERR_WITNESS = -6 /* bbgpu_plonk_set_witness_check is on and a witness does not satisfy the circuit: no proof was written */
};

/* polynomial_arithmetic.hpp:27-41: which member of the fft family */
typedef enum {
    BBGPU_FFT = 0,                     /* fft()                      polynomial_arithmetic.cpp:266 */
    BBGPU_IFFT = 1,                    /* ifft()                     :271-277 */
    BBGPU_COSET_FFT = 2,               /* coset_fft()                :287-291 */
    BBGPU_COSET_IFFT = 3,              /* coset_ifft()               :311-315 */
    BBGPU_FFT_WITH_CONSTANT = 4,       /* fft_with_constant()        :279-285 */
    BBGPU_IFFT_WITH_CONSTANT = 5,      /* ifft_with_constant()       :301-309 */
    BBGPU_COSET_FFT_WITH_CONSTANT = 6  /* coset_fft_with_constant()  :293-299 */
} bbgpu_ntt_kind;

/* ---- lifetime ---------------------------------------------------------------------------------------------------- */
int bbgpu_init(int device);       /* binds the calling process to one GPU (one process per GPU), allocates workspaces */
void bbgpu_shutdown(void);        /* tears down every device context; the process may bind again afterwards */
int bbgpu_device_count(void);

/* ---- several GPUs from one process ---------------------------------------------------------------------------------
 * bbgpu_init_devices binds the process to `count` device contexts, context k on HIP device devices[k].  Entries may repeat: two contexts on one
 * device share nothing but the GPU (own streams, MSM slots, staging buffers, SRS cache).  Call it before any other GPU entry, or after
 * bbgpu_shutdown().  BBGPU_ERR_ARG: null `devices`, count < 1 or > BBGPU_MAX_CONTEXTS, a negative device, a device >= bbgpu_device_count();
 * BBGPU_ERR_HIP without any device; BBGPU_ERR_STATE when the process is already bound to another set of contexts.  bbgpu_init(d) afterwards
 * returns BBGPU_OK when d == devices[0].
 * What is split: ONLY the two host-pointer MSM entries, bbgpu_msm_g1 and bbgpu_msm_g1_batch.  A call of n points uses m = min(count, n / 2^16)
 * contexts (at least 1); context k takes points [n k / m, n (k + 1) / m) of every job, on a worker thread of its own that the library keeps for
 * the life of the binding, and the m partial sums are added on the host -- the point-range split of batched_scalar_multiplications
 * (scalar_multiplication.cpp:703-738), over GPUs instead of threads.  The result is the one-context result, bit for bit.  With m == 1 the call runs
 * on context 0 as it does without this binding.  Everything else -- transforms, polynomial helpers, bbgpu_msm_g1_plain, the device-pointer MSMs
 * and their tickets, SRS handles, the resident prover -- runs on context 0 (bbgpu_plonk_construct_proof_batch too: like the single proof it holds the
 * prover's lock from its first launch to its last byte).
 * Memory: each context caches the slices it was given of a table registered on first sight (1 / m of its points and window tables each);
 * BBGPU_SRS_CACHE_BYTES caps every context's cache on its own.  A table registered EXPLICITLY stays whole on context 0 (its handle serves the
 * device entries); a split call over it uses it there for context 0's slice and the other contexts register their slices on first sight.
 * Settings (bbgpu_set_precompute, bbgpu_set_host_thresholds, bbgpu_set_timing, the exact-mode default of bbgpu_srs_set_validate) apply to every
 * context; the share settings (bbgpu_set_table_share / _point_share) to context 0 only.  A failure in one context is reported as
 * "context k (device d): ..." after every context has drained its work; the next call starts clean. */
#define BBGPU_MAX_CONTEXTS 8
int bbgpu_init_devices(const int* devices, int count);
int bbgpu_num_contexts(void); /* 1 unless bbgpu_init_devices bound more */
const char* bbgpu_last_error(void);
const char* bbgpu_version(void);

/* Device memory the library holds for the life of the process ("one-time" state: excluded from every timed figure, but a shared GPU has to plan for it).
 * Everything here is bounded: the point tables registered on first sight by BBGPU_SRS_CACHE_BYTES (16 GiB, least recently used first; explicitly registered
 * ones until bbgpu_srs_release), the window tables of one SRS by BBGPU_TABLE_MAX_BYTES (64 GiB), the transforms' twiddle / twist tables -- 128 MiB per 2^20
 * domain, 512 MiB per 2^22 -- by BBGPU_NTT_TABLE_BYTES (8 GiB, least recently used domain sizes dropped and rebuilt on demand), the workspaces by the largest
 * call seen (eight MSM slots, scalar staging, transform scratch). */
typedef struct {
    uint64_t srs_points_bytes;    /* resident base points of all live tables */
    uint64_t srs_table_bytes;     /* their pre-shifted window tables */
    uint64_t srs_auto_bytes;      /* of the two above: held by tables registered on first sight (evictable under srs_cache_cap_bytes) */
    uint64_t srs_cache_cap_bytes;
    uint64_t ntt_table_bytes;     /* twiddle / twist / coset tables of the cached domain sizes */
    uint64_t ntt_table_cap_bytes;
    uint64_t ntt_table_sets;      /* how many domain sizes are cached */
    uint64_t msm_workspace_bytes; /* the MSM slots' workspaces (allocated on first use of a slot, sized by its largest MSM) */
    uint64_t staging_bytes;       /* scalar / coefficient staging, transform scratch, polynomial temporaries, the lanes of bbgpu_plonk_construct_proof_batch */
    uint64_t pinned_host_bytes;   /* pinned host memory: staging buffers and the slots' result arrays */
} bbgpu_memory_info;
int bbgpu_memory_stats(bbgpu_memory_info* out);                     /* the sum over every bound context */
int bbgpu_memory_stats_context(int context, bbgpu_memory_info* out); /* one context's share (the transforms' tables are context 0's); BBGPU_ERR_ARG for an unbound context */

/* ---- the error contract on a machine that HAS a GPU: fault injection (testing) ---------------------------------------
 * The reference API has no error channel (assert.hpp:19-23 compiles to nothing, scalar_multiplication.cpp:680-684 prints and returns), so a GPU call
 * that fails in the middle of a proof must leave the library usable and the shim able to answer on the host (SURVEY 8b "Errors").  Every device
 * allocation, every copy of a caller's buffer and every launch check of the library passes one of four host-side funnels; a spec
 *     "alloc:k" | "h2d:k" | "d2h:k" | "launch:k"          (k = 0: the next such call)
 * makes the k-th call of that kind -- counted from the moment the spec is set -- fail ONCE with the error a real failure of that kind returns
 * (out of memory / invalid value / launch failure) without touching the device.  The environment variable BBGPU_FAIL_AT holds the same spec for
 * programs that cannot call this (read once, at the library's first allocation / copy / launch).  NULL or "" disarms.  No kernel reads any of it.
 * bbgpu_fault_stats: how often each funnel was passed since the spec was set, whether the armed failure fired, how many failures the library rode
 * out by itself (an SRS kept without its window tables), the library's live device allocations (count and bytes: after bbgpu_shutdown() both
 * are 0 unless an error path leaked) and the MSM slots still in flight. */
typedef struct {
    uint64_t alloc_calls, h2d_calls, d2h_calls, launch_checks;
    uint64_t armed;            /* 1 while a failure is armed and has not fired yet */
    uint64_t fired;            /* failures injected since the spec was set (0 or 1) */
    uint64_t absorbed;         /* failures the library continued after WITHOUT returning an error (degraded, still on the GPU) */
    uint64_t live_allocations; /* device allocations of the library that are live now */
    uint64_t live_bytes;
    uint64_t slots_pending;    /* MSM slots with work in flight or a result not yet collected */
} bbgpu_fault_info;
int bbgpu_fault_inject(const char* spec);
int bbgpu_fault_stats(bbgpu_fault_info* out);

/* ---- NTT ---------------------------------------------------------------------------------------------------------
 * Drop-in for polynomial_arithmetic::{fft,ifft,coset_fft,coset_ifft,fft_with_constant,ifft_with_constant,
 * coset_fft_with_constant}(fr::field_t* coeffs, const evaluation_domain& domain[, const fr::field_t& constant]):
 * transforms coeffs[0..n) in place.  `constant` (4 limbs, Montgomery) is read for the *_with_constant kinds only.
 * bbgpu_ntt: host buffer (copied to the device and back; n <= 16 is answered on the host, see bbgpu_set_host_thresholds).
 * bbgpu_ntt_device: device-resident buffer, asynchronous on `hip_stream` (a hipStream_t; NULL = the legacy default stream, so a
 * caller working on the null stream is ordered with the transform as with its own kernels).  The same holds
 * for the polynomial helpers below.  The MSM device entries differ: there NULL selects the ticket's own internal NON-BLOCKING stream
 * (that is what lets consecutive MSMs overlap), which has no implicit ordering with the caller's null stream -- d_scalars must be
 * complete before the call (synchronise, or pass the producing stream).
 * Calls on different streams may be in flight together: the library's shared scratch is handed from one stream to the next by an
 * event (they serialise on the device, results are independent of the interleaving). */
int bbgpu_ntt(uint64_t* coeffs, size_t n, int kind, const uint64_t* constant);
int bbgpu_ntt_device(uint64_t* d_coeffs, size_t n, int kind, const uint64_t* constant, void* hip_stream);
/* `batch` (<= 64) transforms of the same size and kind in one set of launches; transform j occupies
 * d_coeffs[j * stride_elems .. j * stride_elems + n) (the prover transforms its three wire / sigma polynomials together) */
int bbgpu_ntt_device_batch(uint64_t* d_coeffs, size_t n, size_t stride_elems, int batch, int kind, const uint64_t* constant, void* hip_stream);

/* ---- MSM ---------------------------------------------------------------------------------------------------------
 * The prover passes the same SRS to every MSM (reference_string.cpp:16-35), laid out as the 2n-entry endomorphism
 * table of generate_pippenger_point_table (scalar_multiplication.cpp:131-140): entry 2i = P_i, entry 2i+1 = (beta x_i,
 * -y_i).  bbgpu_srs_register uploads the n base points (even entries) once and keeps them resident on the GPU in the
 * kernels' working form; it returns a handle >= 0.  Host-pointer MSM calls look the table up by address (and register
 * it on first sight), so sub-slices `points + 2*off` of a registered table are served from the resident copy
 * (batched_scalar_multiplications slices exactly like that, scalar_multiplication.cpp:720-726). */
/* The address is only a hint: every address hit is re-validated against a per-point content fingerprint taken at upload (first, last
 * and 14 evenly spaced rows of the range the caller passes, the spaced rows moving on with every check; only memory inside that range
 * is read).  RESIDUAL WINDOW: a table rewritten IN PLACE only partially -- first and last row unchanged -- is served from the stale
 * resident copy until a sampled row falls into the rewritten part (after k checks a rewritten fraction f survives with probability
 * ~(1 - f)^(14 k)); a caller that edits a slice of a live SRS must release / re-register it.  A table that was registered on
 * first sight and whose memory now holds other points (freed and reused, or refilled in place) is evicted and uploaded again;
 * tables registered on first sight are also evicted least-recently-used beyond BBGPU_SRS_CACHE_BYTES (default 16 GiB of device
 * memory).  A table registered EXPLICITLY keeps its handle until bbgpu_srs_release: mutate it in place only after releasing it
 * (host-pointer calls stop being served from a handle whose contents changed, device-pointer calls by handle cannot notice). */
int bbgpu_srs_register(const uint64_t* points_endo_table, size_t n);
/* EXACT mode for the address-keyed cache (the reference reads the caller's points on every call, scalar_multiplication.cpp:604-617): with
 * full != 0 every host-pointer MSM (bbgpu_msm_g1, bbgpu_msm_g1_batch and the shim entries above them) served from this table re-hashes EVERY row of
 * the range it uses against the fingerprints taken at upload -- on the host, spread over the staging threads, while the call's kernels already run
 * against the resident copy; if a single row differs the copy is dropped (a table registered on first sight is evicted, an explicitly registered one
 * stops serving host-pointer calls; its handle stays valid) and the call runs once more on a fresh upload: identical inputs -> identical outputs on
 * the very next call, whatever part of the table was rewritten.  srs_handle -1 sets the default for tables registered from now on (on first sight
 * or explicitly); the environment variable BBGPU_SRS_VALIDATE=full does the same at start-up.  A table large enough that the call's scalars bypass the staging
 * pool (more than 8 MiB of them: 2^18 points) is checked in the BACKGROUND on the pool's helper threads, from before the upload of the scalars to after the launches.
 * Cost on MI355X + EPYC 9575F (tools/validate_ab.py, profiles/r05_boundary_ab.txt, one box each, alternating): bbgpu_msm_g1 at 2^16 points +0.1 % (0.35 ms either
 * way); at 2^20 points -- 64 MiB of host memory hashed per call -- +5 ... 11 % by box with the default three helper threads (1.70 -> 1.78 ... 1.87 ms; +21 % before
 * the check moved to the background), +2.7 % with BBGPU_STAGE_THREADS=7, +0.1 % with 11; a batch of three 2^20-point jobs over one table +0.8 % (one check per
 * distinct range).  At or above 5 % at the headline size with the default threads, so the DEFAULT STAYS THE 16-ROW SAMPLE and the residual window described above
 * stays with it; a caller that rewrites live tables in place sets the flag (and gives the pool more threads if it has the cores). */
int bbgpu_srs_set_validate(int srs_handle, int full);
/* Registration also builds, on the device, the pre-shifted window tables 2^(c w) * P_i (the reference's
 * generate_pippenger_precompute_table idea, scalar_multiplication.cpp:90-129): W x n x 64 bytes (1 GiB at n = 2^20), so that
 * all digit windows share one bucket set.  On by default from 1024 points on; bbgpu_set_precompute(0) turns it off for
 * tables registered afterwards.  Results are identical either way.
 * The sorted entries of an MSM carry a 24-bit table row, i.e. one table serves 2^24 / W points (2^20 at 15 windows): a LARGER SRS keeps
 * one table per segment of at most that many points (equal segments; 16 GiB of tables at 2^24 points, up to BBGPU_TABLE_MAX_BYTES = 64 GiB,
 * beyond which -- or when the allocation fails -- the points stay resident without tables), and an MSM over it runs as one PIECE per
 * segment it touches, dealt to the ticket's slot and a helper slot, the piece sums added on the host: the reference's own decomposition
 * into point ranges per thread (scalar_multiplication.cpp:703-738).  2^21 / 2^22 / 2^24 points: 2.7 / 5.1 / 18.9 ms on one MI355X.
 * Row- and bucket-range shares (below) are defined on ONE segment. */
void bbgpu_set_precompute(int enabled);
/* Multi-GPU: tables registered after this call keep only the digit windows that rank `rank` of `world` touches when the W x n (window,
 * point) rows are split evenly over the ranks (bbgpu_msm_g1_device_rows_async with rows [W n r / N, W n (r + 1) / N), or whole-window
 * shares inside that range): ceil(W / world) + 1 windows instead of W.  Asking such a table for other windows returns BBGPU_ERR_STATE.
 * (0, 1) restores full tables. */
void bbgpu_set_table_share(int rank, int world);
/* Multi-GPU, split by POINT range (the slicing of scalar_multiplication.cpp:703-738 -- ranges of points per thread, summed at the end -- at the
 * multi-GPU level): rank r of N registers points [n r / N, n (r + 1) / N) as its own SRS and runs bbgpu_msm_g1_device(_async) over the matching
 * scalars; the N results add up to the MSM (bbgpu_g1_sum).  After this call, tables registered pick the window size the WHOLE MSM of
 * world * n points would (17 bits from 2^19 points on) instead of the one for n points.  1 restores the default. */
void bbgpu_set_point_share(int world);
/* number of digit windows an MSM of n points against this table is split into (use this, not bbgpu_msm_num_windows, to
 * shard windows over ranks: a table carries the window size it was built for) */
int bbgpu_srs_num_windows(int srs_handle, size_t n);
int bbgpu_srs_release(int handle);
/* resident tables right now: all, those registered on first sight (evictable), and the device bytes the latter hold (any may be NULL) */
int bbgpu_srs_cache_stats(int* live_entries, int* auto_entries, uint64_t* auto_bytes);
/* io::read_transcript, G1 part (io/io.hpp:36-182): reads `degree - 1` points of an ignition-format transcript file
 * (srs_db/transcript.dat) behind the generator and writes the 2 * degree entry endomorphism table of
 * generate_pippenger_point_table -- the `monomials` array of ReferenceString (reference_string.cpp:16-35) -- ready for
 * bbgpu_srs_register.  Host code; needs no GPU. */
int bbgpu_transcript_read_g1(const char* path, size_t degree, uint64_t* points_endo_table_out);
/* The writer of the same format: the file io::read_transcript(monomials, g2_x, degree, path) accepts for the SRS whose endo table is
 * given -- degree - 1 G1 points (the generator is implicit), then G2 and x * G2 (the verifier's pairing input, io.hpp:171-180) computed
 * here from the secret `x_mont` (Montgomery), then the 64-byte checksum slot the reference never verifies.  Together with
 * bbgpu_srs_generate this stands in for the missing srs_db/transcript.dat of BASELINE configs 2 and 5.  Host code; needs no GPU. */
int bbgpu_transcript_write(const char* path, const uint64_t* points_endo_table, size_t degree, const uint64_t x_mont[4]);
/* device-side generation of the synthetic SRS x^i * G, i < n, straight into a resident table; optionally also written
 * back to the host as the reference-format 2n endo table (may be NULL).  Stands in for the missing srs_db/transcript.dat */
int bbgpu_srs_generate(const uint64_t* x_mont, size_t n, uint64_t* host_endo_table_out);
/* the same for the points x^(first + i) * G, i < n: the slice a rank of an N-way POINT-range split of a larger MSM keeps (rank r of N:
 * first = r n / N; its MSM over the matching slice of the scalars is its partial sum, bench.py --shard points) */
int bbgpu_srs_generate_range(const uint64_t* x_mont, size_t first, size_t n, uint64_t* host_endo_table_out);

/* drop-in for scalar_multiplication::pippenger(scalars, points, n, bucket_width) (:457-476); scalars not modified.
 * out = {x, y, z} normalised, or infinity flag set (n == 0, all-zero scalars).
 * A sum that IS the point at infinity comes back as the clean encoding (all limbs zero, bit 63 of y limb 3 set).  What the reference emits
 * for it is pinned by tests/golden/infinity_commitments.json: g1::normalize() re-sets the flag (group.hpp:450-468) and every other bit of the
 * pair is whatever the CPU algorithm's accumulators held in that run -- it changes with the OpenMP thread count, and through the Fiat-Shamir
 * hash so does the rest of such a proof.  The flag is all there is to reproduce; the reference's Verifier accepts proofs carrying the clean
 * encoding (tests/test_gpu_plonk.py::test_commitments_at_infinity).  Every other result is the unique affine point and is bit-identical.
 * From 2^19 points on the call runs as two point ranges through the two-slot pipeline (the second range's scalars cross the link under the
 * first one's kernels; BBGPU_HOST_MSM_SPLIT).  Host buffers of up to 8 MiB (BBGPU_STAGE_MAX_BYTES) are copied through the library's own
 * pinned staging buffers rather than pinned in place by the runtime (DESIGN_HISTORY.md 1). */
int bbgpu_msm_g1(const uint64_t* scalars, const uint64_t* points_endo_table, size_t n, uint64_t out[12]);
/* the same sum over a PLAIN table: `points` = n affine points, 64 bytes apart -- the argument convention of the reference's
 * pippenger_low_memory(scalars, points, num_points) (scalar_multiplication.cpp:142-262, which applies beta itself; its test allocates
 * exactly n * 64 bytes, test_scalar_multiplication.cpp:164-187) and of round_points.back() in pippenger_precomputed (:478-574,
 * test_scalar_multiplication.cpp:226-262).  Reads exactly n * 64 bytes of `points`; the table is used once and not cached (these
 * are the reference's test / bench entries, not the prover's).  scalars not modified. */
int bbgpu_msm_g1_plain(const uint64_t* scalars, const uint64_t* points, size_t n, uint64_t out[12]);
/* SURVEY 8b "small sizes": the reference's callers include the Verifier's per-proof MSM over ~20 freshly built points
 * (verifier.cpp:359-363) and proofs of n = 4 circuits (test_verifier.cpp:105-122).  Host-pointer MSMs of at most `msm_max_points`
 * points against a table that is not resident, and host-buffer transforms (bbgpu_ntt) of at most `ntt_max_elements` (<= 64)
 * elements, are answered on the host by csrc/host_small.hpp -- no device allocation, copy or launch; results identical.  Defaults
 * 24 / 16 (env BBGPU_HOST_MSM_MAX / BBGPU_HOST_NTT_MAX); 0 / 0 sends every size to the GPU.  Nothing larger ever runs on the host. */
void bbgpu_set_host_thresholds(int msm_max_points, int ntt_max_elements);

/* drop-in for scalar_multiplication::batched_scalar_multiplications(mul_state, num) (:650-772); layout-identical to
 * multiplication_state (scalar_multiplication.hpp:88-94: points@0, scalars@8, num_elements@16, output@32, size 128) */
typedef struct {
    const uint64_t* points;  /* 2n-entry endo table */
    const uint64_t* scalars; /* n scalars */
    size_t num_elements;
    uint64_t _pad;
    uint64_t output[12]; /* written normalised */
} bbgpu_msm_job;
int bbgpu_msm_g1_batch(bbgpu_msm_job* jobs, size_t num_jobs);

/* scalars already resident in HBM (n x 4 limbs), points = a registered SRS handle (first n points, starting at
 * point `offset`).  Windows [window_begin, window_end) of the signed-digit decomposition are processed -- the whole
 * scalar is windows [0, bbgpu_msm_num_windows(n)).  The result is the partial sum over those windows, normalised; partial
 * sums of disjoint window ranges add up to the full MSM (bbgpu_g1_sum).  This is the multi-GPU entry: rank g takes its
 * share of the windows, partial sums are exchanged (RCCL all-gather of 96 bytes per rank) and folded on every rank. */
int bbgpu_msm_num_windows(size_t n);
int bbgpu_msm_g1_device(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, int window_begin,
                        int window_end, uint64_t out[12], void* hip_stream);
/* Asynchronous form: enqueue (returns a ticket >= 0, or a negative error) and collect later.  A ticket is waited for once, by one
 * thread; the wait blocks outside the library's mutex, so other threads keep issuing and collecting meanwhile.  Up to eight MSMs may be in
 * flight; the bucket-reduction tail and host finish of one then overlap the sort/accumulate of the next (DESIGN_HISTORY.md 5), and
 * small latency-bound MSMs (a prover round's three commitments) run side by side.  With hip_stream == NULL each ticket runs
 * on its own internal stream.  An MSM enqueued while another is in flight is laid out for throughput instead of latency (longer
 * accumulation chunks, row / column sums in two steps: DESIGN_HISTORY.md 5, 6 v); the result is the same point either way. */
int bbgpu_msm_g1_device_async(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, int window_begin,
                              int window_end, void* hip_stream);
/* The same with a share that may start and end INSIDE a digit window: rows [row_begin, row_end) of the W x n (window, point) pairs counted
 * window-major, row = w * n + i, 0 <= row_begin < row_end <= W * n with W = bbgpu_srs_num_windows().  Against window tables every pair is
 * one table row feeding the one shared bucket set, so any split of the rows splits the MSM; N ranks taking [W n r / N, W n (r + 1) / N)
 * stay balanced when N does not divide W.  Needs the window tables (bbgpu_srs_has_window_tables() == 1), else BBGPU_ERR_STATE.
 * Collected with bbgpu_msm_g1_wait like any other ticket; the partial sums of a complete split add up to the MSM (bbgpu_g1_sum). */
int bbgpu_msm_g1_device_rows_async(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, uint64_t row_begin, uint64_t row_end,
                                   void* hip_stream);
/* The other way to split one MSM over N ranks (against window tables): share s of N keeps the digits whose BUCKET falls into its 1 / N of
 * the bucket range -- all windows, all points.  Every share then holds 1 / N of the mixed additions AND 1 / N of the buckets to merge
 * and fold (a row share repeats that tail in full on every rank), at the price of every rank scanning all digits and keeping all window
 * tables (no bbgpu_set_table_share).  Balanced for uniform digits; the partial sums of shares 0 .. N-1 add up to the MSM (bbgpu_g1_sum).
 * N <= the rows of the bucket matrix (256 at 17-bit windows).  Replaces the slicing of scalar_multiplication.cpp:703-738 (there: ranges of
 * POINTS per thread, summed at the end) at the multi-GPU level. */
int bbgpu_msm_g1_device_buckets_async(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, int share, int share_count, void* hip_stream);
int bbgpu_srs_has_window_tables(int srs_handle); /* 1 / 0, < 0: unknown handle */
int bbgpu_msm_g1_wait(int ticket, uint64_t out[12]);
/* Whole-batch entry (the prover commits 3 / 1 / 3 / 2 polynomials per round over the same SRS,
 * prover.cpp:65-122,650-658): `jobs` (1..4) resident scalar vectors of n scalars each against points [offset, offset + n) of a
 * table registered WITH window tables, issued as ONE pass through the pipeline (per table segment touched) -- one bucket set per job in
 * the shared sort / accumulate / merge / reduction kernels -- so the batch pays one chain of launches and dependent additions, not `jobs`.
 * bbgpu_msm_g1_batch_wait writes jobs x 12 limbs (normalised).  Uses one of the eight tickets (and, over several segments, a free
 * one as its helper). */
int bbgpu_msm_g1_device_batch_async(int srs_handle, size_t offset, const uint64_t* const* d_scalars, int jobs, size_t n, void* hip_stream);
int bbgpu_msm_g1_batch_wait(int ticket, uint64_t* out);
/* out = sum of `count` normalised/Jacobian points (infinity flags honoured), normalised.  Host arithmetic. */
int bbgpu_g1_sum(const uint64_t* points12, size_t count, uint64_t out[12]);

/* ---- resident polynomial helpers -------------------------------------------------------------------
 * The O(n) loops of the prover that sit between the transforms and the commitments, on device-resident vectors in the
 * reference's memory format (n x 4 limbs, Montgomery; any representative below 2^256 in, canonical out).  All are
 * asynchronous on `hip_stream` (NULL = the legacy default stream) except where a host value is returned. */
/* polynomial_arithmetic::evaluate(coeffs, z, n) (polynomial_arithmetic.cpp:337-373): sum_i coeffs[i] z^i, canonical */
int bbgpu_fr_evaluate_device(const uint64_t* d_coeffs, size_t n, const uint64_t z[4], uint64_t out[4], void* hip_stream);
/* fr::batch_invert(coeffs, n) (fields/field.hpp:503-522), in place; every element must be non-zero */
int bbgpu_fr_batch_invert_device(uint64_t* d_values, size_t n, void* hip_stream);
/* running products (the six accumulator chains of prover.cpp:194-202 are the exclusive prefix form):
 * out[i] = prod of in[j] over j < i (exclusive) or j <= i (inclusive); reverse != 0 scans from the top (j > i / j >= i) */
int bbgpu_fr_product_scan_device(const uint64_t* d_in, uint64_t* d_out, size_t n, int reverse, int inclusive, void* hip_stream);
/* polynomial_arithmetic::mul(a, b, r, domain) (:328-335) */
int bbgpu_fr_mul_device(uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n, void* hip_stream);
/* polynomial_arithmetic::compute_kate_opening_coefficients(src, dest, z, n) (:562-591): dest = (F(X) - F(z)) / (X - z),
 * returns F(z) in f_of_z (may be NULL).  dest may alias src only if it IS src. */
int bbgpu_kate_opening_device(const uint64_t* d_src, uint64_t* d_dest, size_t n, const uint64_t z[4], uint64_t f_of_z[4], void* hip_stream);
/* polynomial_arithmetic::compute_lagrange_polynomial_fft(l_1, src_domain, target_domain) (:381-476): n_target values */
int bbgpu_lagrange_l1_fft_device(uint64_t* d_l_1, size_t n_src, size_t n_target, void* hip_stream);
/* polynomial_arithmetic::divide_by_pseudo_vanishing_polynomial(coeffs, src_domain, target_domain) (:478-560), in place */
int bbgpu_divide_by_pseudo_vanishing_device(uint64_t* d_coeffs, size_t n_src, size_t n_target, void* hip_stream);
/* waffle::compute_permutation_lagrange_base_single(output, permutation, small_domain) (permutation.hpp:15-87) */
int bbgpu_permutation_lagrange_base_device(uint64_t* d_out, const uint32_t* d_mapping, size_t n, void* hip_stream);

/* Evaluation and opening in evaluation form: `batch` polynomials of degree < n given by their VALUES v_i = f(w^i) on the size-n domain (w =
 * fr_root_of_unity(log2 n), the root the transforms and bbgpu_srs_lagrange use), value i of polynomial b at d_values[(b * stride_elems + i) * 4], at one
 * point z -- without the inverse transform the coefficient-form entries above need first.  The reference has no counterpart.  For z outside the domain
 *   f(z) = (z^n - 1) / n * sum_i v_i w^i / (z - w^i)          q_i = (f(z) - v_i) / (z - w^i)
 * and for z = w^m:  f(z) = v_m,  q_i = (v_m - v_i) / (z - w^i) for i != m,  q_m = -sum_{i != m} q_i w^(i - m).  The host decides which case holds before
 * anything is launched (z reduced, z^n == 1 by log2 n squarings, then m bit by bit), so z on the domain -- given as any representative, w^m + r
 * included -- is legal and exact.
 *   out / f_of_z  batch x 4 words of HOST memory: bit for bit what bbgpu_fr_evaluate_device returns for ifft(values_b).  f_of_z may be NULL.
 *   d_quotient    the values of (f_b(X) - f_b(z)) / (X - z) on the domain, in the layout (and with the stride) of d_values: bit for bit the fft of what
 *                 bbgpu_kate_opening_device writes for ifft(values_b), so its commitment over a bbgpu_srs_lagrange handle is the opening proof.  It may
 *                 alias d_values only if it IS d_values; elements between the polynomials (stride_elems > n) are neither read nor written.
 *   errors        BBGPU_ERR_SIZE: n not a power of two in [2, 2^24], batch outside 1..64, stride_elems < n; BBGPU_ERR_ARG: null d_values, d_quotient, z
 *                 or out -- all refused before a device is bound.  The device pointers themselves are the caller's responsibility, as for every helper
 *                 of this section: they are not validated.
 * One inversion per call, shared by the polynomials of the batch (csrc/poly.hip bary_open: k_bary_denominators, the batch inversion of
 * bbgpu_fr_batch_invert_device, k_bary_dot + k_bary_finish, k_bary_quotient; the powers of w are made in the lanes, no table of roots is kept or read).
 * The batch inversion synchronises the stream ONCE for its host inversion, so these entries are not fully asynchronous; when f_of_z == NULL nothing else
 * synchronises, otherwise one read-back does.  bbgpu_fr_evaluate_lagrange_device at z on the domain is a copy of v_m alone.  They run on context 0 and use
 * the library's polynomial scratch (bbgpu_memory_info.staging_bytes: about 3 n x 32 bytes + 8 KiB per polynomial of the batch); they keep no per-domain table.
 * Every allocation, read-back and launch check passes the fault-injection funnels (a warm call: no allocation, no upload, one read-back when values are
 * returned, five launch checks -- the denominators, the two scans and the scaling of the inversion, the chain of dot, finish and quotient).
 * Cost on one MI355X (tools/lagrange_open_bench.py, profiles/lagrange_open.txt; wall ms per call sequence, these entries against the PARENT library's
 * bbgpu_ntt_device_batch(IFFT) + one coefficient-form entry per polynomial, alternating in one process; the transform path is not charged the copy that
 * keeping the values would cost):
 *                                 2^16 values                      2^20 values
 *                            batch 1         batch 8          batch 1         batch 8
 *   evaluate              0.182 / 0.083   0.187 / 0.418    0.351 / 0.163   0.554 / 1.120
 *   open                  0.189 / 0.130   0.202 / 0.773    0.374 / 0.266   0.723 / 1.932
 *   open + commitments    0.472 / 0.420   2.251 / 2.826    1.645 / 1.551   10.76 / 12.03
 * Evaluate, batch 1: the transform path wins at both sizes (by 0.10 and 0.19 ms) -- a call here is the batch inversion, two product scans and a
 * synchronisation, against a transform of 0.03 .. 0.1 ms; a caller with ONE polynomial should take IFFT + bbgpu_fr_evaluate_device.  Evaluate, batch 8:
 * this entry wins (2.2x and 2.0x): the inversion is shared, its time hardly grows with the batch, the other path pays per polynomial.  Open, batch 1: the
 * transform path wins again (by 0.06 and 0.11 ms), and still does with the commitment behind it (by 0.05 and 0.09 ms, beyond the spreads of 0.02 and
 * 0.06): take IFFT + bbgpu_kate_opening_device for one polynomial when the monomial table is resident anyway.  Open, batch 8: this entry wins (3.8x and
 * 2.7x; by 0.58 and 1.27 ms of a call sequence that the eight MSMs dominate once the commitments are counted).  What the entries buy at
 * batch 1 is not time: the monomial table and the transform's tables need not be resident. */
int bbgpu_fr_evaluate_lagrange_device(const uint64_t* d_values, size_t n, size_t stride_elems, int batch, const uint64_t z[4],
                                      uint64_t* out /* batch x 4, host */, void* hip_stream);
int bbgpu_kate_opening_lagrange_device(const uint64_t* d_values, uint64_t* d_quotient, size_t n, size_t stride_elems, int batch, const uint64_t z[4],
                                       uint64_t* f_of_z /* batch x 4, host; may be NULL */, void* hip_stream);

/* Opening sessions: the same two operations at SEVERAL points over one shared inversion, and the opening of a FOLD of polynomials.  The two entries above
 * spend most of a call on the batch inversion and throw the inverses 1 / (z - w^i) away; a prover that opens at z and z w (as PLONK does), or evaluates
 * first to derive its folding challenge and opens afterwards, pays it two or four times, and commits to one quotient per polynomial.  A session makes the
 * inverses of up to BBGPU_OPENING_MAX_POINTS points ONCE and keeps them; every pairing-based protocol then folds the polynomials opened at one point with
 * challenge multipliers and commits to ONE quotient per point -- the quotient is linear in the polynomial.  Domain, root, value layout and the on-domain
 * rules are those of the two entries above; all field elements are in the reference's memory format, any representative in, canonical out.
 *   begin        z: points x 4 words of HOST memory.  Every z_t is reduced and judged on the host (on the domain, and where) as above; ONE launch writes the
 *                denominators of all points, point-major (k_bary_denominators, one grid row per point, z_t and m_t by value), ONE batch inversion
 *                inverts them -- one host inversion and one synchronisation for the whole session.  Equal points are legal.  Returns a handle >= 0.  The
 *                inverses (points x n x 32 bytes) live in an allocation of the session's own, counted in bbgpu_memory_info.staging_bytes, released by end
 *                and by bbgpu_shutdown.  BBGPU_ERR_SIZE: n not a power of two in [2, 2^24], points outside 1..4, points x n > 2^24; BBGPU_ERR_ARG: null z;
 *                BBGPU_ERR_STATE: BBGPU_OPENING_MAX_SESSIONS sessions are live -- all refused before a device is bound.  After a failed begin no session
 *                exists and nothing it allocated is live.
 *   evaluate     bit for bit what bbgpu_fr_evaluate_lagrange_device returns for the same values at the session's z_point, without denominators or an
 *                inversion: off the domain k_bary_dot and k_bary_finish, on it the copy of v_m alone; one read-back synchronises.
 *   open         bit for bit bbgpu_kate_opening_lagrange_device, the in-place rule and the untouched padding included: off the domain dot, finish,
 *                quotient; on it stash, quotient, dot, finish.  With f_of_z == NULL it synchronises nothing.
 *   open_folded  with F = sum_b gamma_b f_b (gamma: batch x 4 words of HOST memory), d_quotient[i], n elements, is set -- or, with accumulate != 0, added
 *                to, canonically -- to the values of (F(X) - F(z)) / (X - z) on the domain, element m for z = w^m included (the rule above applied to F);
 *                folded_f_of_z (may be NULL) = F(z), the F of this call alone.  accumulate == 0 writes every one of the n elements.  d_quotient must not
 *                overlap d_values (not validated, like every device pointer of this section).  The quotient is linear: several calls with accumulate fold
 *                polynomials that live in different buffers or strides into one proof.  The batch x n values are read ONCE: off the domain k_bary_fold_dot
 *                forms F_i (one shared reduction per term), stores it and sums F_i w^i inv_i in the same trip, then k_bary_finish and k_bary_quotient
 *                run in place on the n elements; on the domain k_fold, the copy of F_m, quotient, dot, finish.  When accumulating, F and its quotient are
 *                made in the scratch and one more pass over n elements adds them to d_quotient.
 *   end          releases the session; BBGPU_ERR_ARG for a handle that is not live.
 * The four session calls refuse without touching a device: BBGPU_ERR_SIZE for batch outside 1..64 or stride_elems < n, BBGPU_ERR_ARG for an unknown
 * session, a point outside the session or a null pointer the call needs.  They run on context 0 under the library mutex; every allocation, read-back and
 * launch check passes the fault-injection funnels (warm calls at n = 4096, DESIGN.md 7 -- begin: one allocation, four launch checks, the denominators and
 * the inversion's three; evaluate: one launch check off the domain, none on it, one read-back; open: one launch check, one read-back when f_of_z is
 * wanted; open_folded: one launch check, two when accumulating, one read-back when folded_f_of_z is wanted; no upload anywhere).  After a failed call the
 * session stays usable.
 * Cost on one MI355X (tools/opening_session_bench.py, profiles/opening_session.txt; wall ms per call sequence, this library against the PARENT library in
 * one process, alternating pairs, medians of 21, spreads as interquartile ranges).  The PLONK shape: eight polynomials, six opened at z and two at z w, all
 * evaluations wanted, one proof point per point -- parent: two bbgpu_kate_opening_lagrange_device calls and eight MSMs; session: begin(2 points), two
 * evaluate, two open_folded, two MSMs, end.  One polynomial: begin + evaluate + end against the parent's entry and against IFFT + bbgpu_fr_evaluate_device.
 *                                          2^16 values                  2^20 values
 *                                      session / parent              session / parent
 *   PLONK shape + commitments          1.210 / 2.444                 3.786 / 10.93          session lower, by 1.23 and 7.14 ms (spreads 0.04, 0.12)
 *   PLONK shape, no commitments        0.611 / 0.392                 1.255 / 1.011          PARENT lower, by 0.22 and 0.24 ms (spreads 0.006, 0.011)
 *   evaluate one polynomial            0.198 / 0.181  (IFFT: 0.086)  0.534 / 0.345  (IFFT: 0.167)   parent lower by 0.02 and 0.19 ms, the transform path lowest
 * With the commitments the sequence falls by the six MSMs saved, as expected (2.0x and 2.9x).  WITHOUT them it goes the other way: the expectation that
 * it falls by about one inversion is refuted.  The calls alone (the same file): begin(2 points) + end 0.338 / 0.622 ms around a batch inversion of 2 n elements
 * that takes 0.118 / 0.355 -- the session's own allocation, a hipMalloc and a hipFree that waits for the device, costs 0.2 .. 0.3 ms, more than the inversion
 * it saves (0.1 .. 0.2 ms) -- and the four session calls cost 0.064 + 0.062 + 0.096 + 0.073 ms at 2^16 and 0.212 + 0.102 + 0.175 + 0.119 at 2^20, two of
 * them (the evaluations) a synchronisation each that the parent's two calls do not make.  (At 2^16 the allocation's cost is bimodal between runs: the same
 * begin + evaluate + end measured 0.198 in one pairing and 0.382 in the next.)  A caller who needs the values before the folding challenge has no
 * alternative to evaluating first; one who opens a single point without folding and commits per polynomial should stay with the entries above.  Nothing
 * was tuned after these measurements.  The two existing entries, parent against child in the same run, agree within 0.007 ms in every cell (batch 1 and 8,
 * both sizes), inside the spreads.
 */
#define BBGPU_OPENING_MAX_POINTS 4
#define BBGPU_OPENING_MAX_SESSIONS 16
int bbgpu_lagrange_opening_begin(size_t n, const uint64_t* z /* points x 4, host */, int points, void* hip_stream); /* session handle >= 0 */
int bbgpu_lagrange_opening_evaluate(int session, int point, const uint64_t* d_values, size_t stride_elems, int batch,
                                    uint64_t* out /* batch x 4, host */, void* hip_stream);
int bbgpu_lagrange_opening_open(int session, int point, const uint64_t* d_values, uint64_t* d_quotient, size_t stride_elems, int batch,
                                uint64_t* f_of_z /* batch x 4, host; may be NULL */, void* hip_stream);
int bbgpu_lagrange_opening_open_folded(int session, int point, const uint64_t* d_values, size_t stride_elems, int batch,
                                       const uint64_t* gamma /* batch x 4, host */, uint64_t* d_quotient /* n elements */, int accumulate,
                                       uint64_t folded_f_of_z[4] /* host; may be NULL */, void* hip_stream);
int bbgpu_lagrange_opening_end(int session);
/* The fold alone: d_out[i] is set (accumulate == 0) or added to sum_b gamma_b v_{b,i}, canonical, asynchronous (k_fold, one launch): what a prover folds
 * beside the quotient.  1 <= n <= 2^24, not necessarily a power of two; batch 1..64; stride_elems >= n (else BBGPU_ERR_SIZE); BBGPU_ERR_ARG for a null
 * pointer; both before a device is bound.  d_out must not overlap d_values. */
int bbgpu_fr_fold_device(uint64_t* d_out /* n */, const uint64_t* d_values, size_t n, size_t stride_elems, int batch,
                         const uint64_t* gamma /* batch x 4, host */, int accumulate, void* hip_stream);

/* The same on host buffers (copied to the device and back): what the C++ shim forwards the co-resident functions of the replaced
 * translation unit to, so that polynomial_arithmetic.o / scalar_multiplication.o can be left out of the link altogether. */
int bbgpu_fr_evaluate(const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t out[4]);
int bbgpu_kate_opening(const uint64_t* src, uint64_t* dest, size_t n, const uint64_t z[4], uint64_t f_of_z[4]);
int bbgpu_lagrange_l1_fft(uint64_t* l_1, size_t n_src, size_t n_target);
int bbgpu_divide_by_pseudo_vanishing(uint64_t* coeffs, size_t n_src, size_t n_target);
/* polynomial_arithmetic::get_lagrange_evaluations(z, domain) (:594-626): out = {Z_H*(z), L_1(z), L_{n-1}(z)}; host arithmetic */
int bbgpu_lagrange_evaluations(const uint64_t z[4], size_t n, uint64_t out[12]);
/* scalar_multiplication::generate_pippenger_point_table(points, table, n) (scalar_multiplication.cpp:131-140); points may alias table */
int bbgpu_generate_point_table(const uint64_t* points, uint64_t* table, size_t n);

/* ---- resident PLONK prover (BASELINE config 5) ------------------------------------------------------
 * waffle::Prover for the standard arithmetic circuit with every polynomial resident in HBM.  The circuit description is
 * the state StandardComposer::preprocess() hands the reference's Prover (standard_composer.cpp:163-220, prover.hpp:44-59,
 * widgets/arithmetic_widget.hpp:45-49): per-gate wire VALUES, the three sigma permutation mappings (low bits: gate index,
 * bits 30-31: 0 left / 1 right / 2 output wire) and the five selector VALUES, all of length n = 2^k.  The SRS is a registered
 * / generated handle holding at least n points (monomials[i] = x^i G, reference_string.cpp:16-35). */
typedef struct {
    size_t n;
    const uint64_t *w_l, *w_r, *w_o;                                   /* n x 4 limbs each */
    const uint32_t *sigma_1_mapping, *sigma_2_mapping, *sigma_3_mapping; /* n each */
    const uint64_t *q_m, *q_l, *q_r, *q_o, *q_c;                       /* n x 4 limbs each */
    /* optional second widget, all three or none (NULL): the boolean-constraint selectors BoolComposer::preprocess() hands
     * ProverBoolWidget (bool_composer.cpp:68-143, widgets/bool_widget.hpp): q_bl, q_br, q_bo, n x 4 limbs each */
    const uint64_t *q_bl, *q_br, *q_bo;
    /* or (not both) the MiMC widget's selectors as MiMCComposer::preprocess() hands ProverMiMCWidget (mimc_composer.cpp:170-250,
     * widgets/mimc_widget.hpp): q_mimc_selector, q_mimc_coefficient (the round constants), n x 4 limbs each; NULL without it.
     * The proof then also carries w_o_shifted_eval and q_mimc_coefficient_eval. */
    const uint64_t *q_mimc_selector, *q_mimc_coefficient;
    /* optional sequential widget (ExtendedComposer::preprocess(), extended_composer.cpp:460-607, widgets/sequential_widget.hpp): q_o_next,
     * the selector of the NEXT gate's output wire in the arithmetic identity, n x 4 limbs; NULL without it.  May be combined with the
     * bool widget (the ExtendedComposer's chain: arithmetic, sequential, bool), not with the MiMC widget.  The proof then carries
     * w_o_shifted_eval. */
    const uint64_t *q_o_next;
} bbgpu_plonk_circuit;
/* proof = waffle::plonk_proof (waffle_types.hpp:18-45) in its own field order: W_L, W_R, W_O, Z_1, T_LO, T_MID, T_HI,
 * PI_Z, PI_Z_OMEGA (affine x, y: 8 limbs each), then w_l_eval, w_r_eval, w_o_eval, sigma_1_eval, sigma_2_eval,
 * z_1_shifted_eval, linear_eval, and the widget-dependent w_l_shifted_eval, w_r_shifted_eval, w_o_shifted_eval, q_c_eval,
 * q_mimc_coefficient_eval (4 limbs each; zero unless a widget fills them: the MiMC widget sets w_o_shifted_eval and
 * q_mimc_coefficient_eval, the sequential widget w_o_shifted_eval); Montgomery form, canonical -- byte-identical to the reference's proof */
#define BBGPU_PLONK_PROOF_WORDS 120
int bbgpu_plonk_prover_create(const bbgpu_plonk_circuit* circuit, int srs_handle); /* returns a prover handle >= 0 */
int bbgpu_plonk_prover_set_witness(int prover, const uint64_t* w_l, const uint64_t* w_r, const uint64_t* w_o);
/* Prover::construct_proof (prover.cpp:661-670) of the witness the handle holds.  It is a batch of one over a lane of the handle's own (see
 * bbgpu_plonk_construct_proof_batch below): the same rounds, kernels and copies, so it passes the "h2d" / "d2h" funnels of bbgpu_fault_inject as a batch
 * does -- the records its kernels read are uploaded, its evaluations read back, through them.  On a failure proof_out is not written, no MSM ticket is
 * outstanding and the handle stays usable.  It touches neither bbgpu_plonk_batch_challenges nor bbgpu_plonk_last_batch_timing. */
int bbgpu_plonk_construct_proof(int prover, uint64_t proof_out[BBGPU_PLONK_PROOF_WORDS]);
/* waffle::preprocess(prover) (preprocess.hpp:16-55, arithmetic_widget.cpp:128-157, bool_widget.cpp:118-152): the verification key of
 * the circuit -- SIGMA_1, SIGMA_2, SIGMA_3, the commitments to q_m, q_l, q_r, q_o, q_c, and with the bool widget those to q_bl, q_br,
 * q_bo, with the MiMC widget q_mimc_coefficient, q_mimc_selector, with the sequential widget q_o_next (before the bool widget's three) --
 * affine x, y: 8 limbs each; 8 to 12 points, pass room for 12 */
#define BBGPU_PLONK_VK_WORDS 96
int bbgpu_plonk_preprocess(int prover, uint64_t vk_out[BBGPU_PLONK_VK_WORDS]);
int bbgpu_plonk_last_challenges(int prover, uint64_t out[20]); /* beta, gamma, alpha, z, nu (waffle_types.hpp:9-16) */
int bbgpu_plonk_last_timing(int prover, double ms_out[4]);     /* construct_proof wall ms: total, in commitments, rest, first-use preparation */
/* A batch of proofs of the prover's circuit, one per witness, in one call: the rounds of construct_proof advance in lockstep over `count` LANES, every
 * round step one launch for all lanes, the commitments of a round as batch tickets side by side -- the chip is mostly idle inside one proof of up to
 * about 2^18 gates, and only another proof's work can fill it (each round waits for its own Fiat-Shamir challenge).
 * w_l[j], w_r[j], w_o[j]: host arrays of n x 4 limbs (the format of bbgpu_plonk_prover_set_witness).  proofs_out: count x BBGPU_PLONK_PROOF_WORDS;
 * proof j is, byte for byte, what bbgpu_plonk_prover_set_witness(w_l[j], w_r[j], w_o[j]) + bbgpu_plonk_construct_proof would return.
 * BBGPU_ERR_ARG: unknown handle, count < 1, count > BBGPU_PLONK_MAX_BATCH, a null array or a null entry; BBGPU_ERR_SIZE: count * n > 2^22 (the lanes
 * hold 48 vectors of n x 32 bytes each: 96 MiB per lane at 2^16 gates, 6 GiB at the bound).  These checks come before the library binds a device.
 * The batch lanes are allocated on the first batch, grown when a larger count arrives, released with the handle, and counted in
 * bbgpu_memory_info.staging_bytes (the handle's own lane, which the single entries use, is part of the handle from its creation).  The call touches neither the witness the handle holds for bbgpu_plonk_construct_proof nor
 * bbgpu_plonk_last_challenges / _last_timing.  On a failure every MSM ticket the call issued has been collected and the handle stays usable. */
#define BBGPU_PLONK_MAX_BATCH 16
int bbgpu_plonk_construct_proof_batch(int prover, int count, const uint64_t* const* w_l, const uint64_t* const* w_r, const uint64_t* const* w_o,
                                      uint64_t* proofs_out);
int bbgpu_plonk_batch_challenges(int prover, int lane, uint64_t out[20]); /* beta, gamma, alpha, z, nu of lane `lane` of the last batch */
int bbgpu_plonk_last_batch_timing(int prover, double ms_out[4]);          /* as bbgpu_plonk_last_timing, for the whole batch */
/* ---- does a witness satisfy the circuit?  (checked on the GPU before proving; the reference has no such check) ------
 * The prover takes any witness: for one that violates the circuit it returns BBGPU_OK and 960 bytes the Verifier rejects (Prover::construct_proof
 * divides by the vanishing polynomial blindly, and so do the entries above).  These entries answer the question exactly, and say where.
 * What "satisfies" means is what the proof system enforces.  It divides every identity by the PSEUDO vanishing polynomial
 * Z_H*(X) = (X^n - 1) / (X - w^(n-1)) (polynomial_arithmetic.cpp:478-560), and the grand product runs over rows 0 .. n-2 with Z(w^(n-1)) = 1 enforced by
 * the L_{n-1} term (prover.cpp:135-222, :364-398): ROW n-1 IS NOT CONSTRAINED, neither its gate identity nor its copy constraints, and the Verifier
 * accepts whatever stands there (all composers but one leave a padding row, new_n >= n + 1; MiMCComposer::preprocess rounds n itself, and the
 * Verifier rejects its honest proof when the gate count is a power of two -- two wire cycles then run through row n-1, which the check reports).
 * With R = n - 1, rows i = 0 .. R-1, all arithmetic modulo r on any representative below 2^256:
 *   gate identities, each zero on its own (the widgets separate them by powers of alpha):
 *     ARITH      q_m w_l w_r + q_l w_l + q_r w_r + q_o w_o + q_c  (+ q_o_next[i] w_o[i+1] with the sequential widget, sequential_widget.cpp:47-62)
 *     BOOL_L/R/O q_bl (w_l^2 - w_l), q_br (w_r^2 - w_r), q_bo (w_o^2 - w_o)                                     (bool_widget.cpp:62-100)
 *     MIMC_CUBE  q_mimc_selector (t^3 - w_r),  MIMC_OUT  q_mimc_selector (t w_r^2 - w_o[i+1]),  t = w_o + w_l + q_mimc_coefficient  (mimc_widget.cpp:68-85)
 *   copy constraints: for each of the 3R wire positions p = (row i < R, wire k) with the mapping entry m decoded as the prover decodes it
 *     (row = (m & (2^29 - 1)) & (n - 1), wire = bits 30-31, code 3 read as the left wire): the value at sigma(p) equals the value at p modulo r, AND
 *     sigma(p) lies in a row < R (a position whose sigma points into row n-1 breaks the grand product as surely as unequal values do).
 * Whether the three mappings form a permutation is a property of the circuit, not of a witness, and is not checked. */
#define BBGPU_PLONK_FAIL_ARITH 1u
#define BBGPU_PLONK_FAIL_BOOL_L 2u
#define BBGPU_PLONK_FAIL_BOOL_R 4u
#define BBGPU_PLONK_FAIL_BOOL_O 8u
#define BBGPU_PLONK_FAIL_MIMC_CUBE 16u
#define BBGPU_PLONK_FAIL_MIMC_OUT 32u
#define BBGPU_PLONK_NONE 0xFFFFFFFFu
typedef struct {
    uint64_t gate_failures;     /* rows < n-1 in which at least one identity is non-zero */
    uint64_t copy_failures;     /* wire positions in rows < n-1 that fail their copy constraint */
    uint32_t first_gate;        /* smallest failing row, BBGPU_PLONK_NONE if none */
    uint32_t first_gate_kinds;  /* the identities failing in that row (bit mask), 0 if none */
    uint32_t kinds;             /* OR of the masks of all failing rows */
    uint32_t first_copy;        /* first failing position in mapping encoding (row | wire << 30), ordered by row, then wire; BBGPU_PLONK_NONE if none */
    uint32_t first_copy_target; /* its mapping entry, BBGPU_PLONK_NONE if none */
    uint32_t _pad;
} bbgpu_plonk_witness_report;
/* A witness is good iff gate_failures == 0 && copy_failures == 0.  Both entries return BBGPU_OK when the check RAN; the verdict is in the report.  The
 * reports do not vary from run to run and equal bbgpu_host_plonk_check_witness's, field for field.  Two launches per call however many lanes.
 * bbgpu_plonk_check_witness: the witness the handle holds (bbgpu_plonk_prover_create / _set_witness).
 * bbgpu_plonk_check_witness_batch: `count` witnesses as bbgpu_plonk_construct_proof_batch takes them, one report each; the same argument and size rules,
 * refused before a device is bound.  The witnesses are uploaded into the lanes of the batch entry, so a following batch proof of the same count
 * allocates nothing new.  Neither entry touches the witness the handle holds, its challenges or its timings. */
int bbgpu_plonk_check_witness(int prover, bbgpu_plonk_witness_report* out);
int bbgpu_plonk_check_witness_batch(int prover, int count, const uint64_t* const* w_l, const uint64_t* const* w_r, const uint64_t* const* w_o,
                                    bbgpu_plonk_witness_report* out /* count */);
/* enabled != 0: bbgpu_plonk_construct_proof and bbgpu_plonk_construct_proof_batch check the witness(es) they are about to prove -- the same kernels on the
 * vectors already uploaded -- before the first commitment.  If any lane fails, the call returns BBGPU_ERR_WITNESS, writes NO proof bytes for any lane, has
 * no MSM ticket outstanding and leaves the handle usable; bbgpu_last_error() names the first bad lane, row and kind, bbgpu_plonk_last_witness_report gives
 * every lane's report (lane 0 for the single proof).  The caller drops the bad lanes and calls again.  Default 0: nothing is checked, launched or copied
 * that was not before. */
int bbgpu_plonk_set_witness_check(int prover, int enabled);
int bbgpu_plonk_last_witness_report(int prover, int lane, bbgpu_plonk_witness_report* out); /* of the last checked proof call or check entry */
/* ---- witnesses as composer variables, from host or device memory --------------------------------------------------
 * The entries above take a witness as three expanded wire vectors in host memory.  Those exist only after Composer::preprocess() has run the loop
 * output_state.w_l[i] = variables[w_l[i]] (standard_composer.cpp:205-209; the bool, MiMC and extended composers have the same loop), and two thirds of
 * their bytes are repeats: the circuit -- selectors, mappings AND the wire -> variable indices -- is the same for every witness, only the composer's
 * `variables` differ.  With a wire map on the handle a witness is its variables, and the loop runs on the GPU, one launch for all lanes.
 * bbgpu_plonk_prover_set_wire_map: the indices the composer holds (ComposerBase::w_l / w_r / w_o after preprocess() padded them with zero_idx), n
 * entries each, every entry < num_variables.  A property of the circuit: set once per handle (a second call replaces the map).
 * BBGPU_ERR_ARG: a null array; an index >= num_variables (the message names the wire and the first such row: checked here, once, on the host, so that
 * no kernel ever reads outside the variables).  BBGPU_ERR_SIZE: num_variables 0 or > 4 n (a map references at most 3 n variables; the slack is for
 * variables no gate uses, e.g. after assert_equal; the bound sizes the per-lane staging).  All of that comes before the library binds a device. */
int bbgpu_plonk_prover_set_wire_map(int prover, const uint32_t* w_l_index, const uint32_t* w_r_index, const uint32_t* w_o_index, size_t num_variables);
enum { BBGPU_PLONK_WITNESS_WIRES = 0, BBGPU_PLONK_WITNESS_VARIABLES = 1 }; /* form  */
enum { BBGPU_PLONK_WITNESS_HOST = 0, BBGPU_PLONK_WITNESS_DEVICE = 1 };     /* where */
typedef struct {
    int form, where;
    const uint64_t *w_l, *w_r, *w_o; /* WIRES: n x 4 limbs each (as bbgpu_plonk_prover_set_witness) */
    const uint64_t* variables;       /* VARIABLES: num_variables x 4 limbs, Montgomery, any representative below 2^256 (copied bit for bit) */
    void* hip_stream;                /* DEVICE: the stream the data was produced on (NULL = the legacy default stream) */
} bbgpu_plonk_witness;
/* The three witness-taking entries for a witness in any form and place; lanes of one batch may mix them.  WIRES / HOST is exactly the path of the entries
 * above (the same uploads, launches and bytes); every other kind yields, byte for byte, the proof / report of the expanded wires.  Everything else --
 * bbgpu_plonk_set_witness_check, _last_witness_report, _batch_challenges, _last_batch_timing, count <= BBGPU_PLONK_MAX_BATCH, count * n <= 2^22 -- applies
 * unchanged.  BBGPU_ERR_ARG: a null descriptor, a null pointer the form needs, an unknown form or where (refused before a device is bound);
 * BBGPU_ERR_STATE: VARIABLES on a handle without a wire map.
 * DEVICE pointers are dereferenced by kernels, and with XNACK off a pointer the device cannot reach faults the card: each is looked up in the runtime
 * before anything is enqueued and must be 16-byte aligned device memory of the prover's device (context 0's) that holds the whole vector, else
 * BBGPU_ERR_ARG.  "Holds the whole vector" is judged against the runtime's allocation (hipMemGetAddressRange; a pointer whose allocation the runtime
 * cannot bound is refused): a sub-allocation of a caching allocator -- a tensor shorter than the vector inside a larger block -- passes, its length is
 * the caller's to get right.  The library records an event on hip_stream and lets the prover's stream wait for it, so hip_stream must be a live stream
 * of the prover's device (NULL = the legacy default stream); it is not validated, a stale handle or a stream of another device is the runtime's error
 * (BBGPU_ERR_HIP), reported after the pointer checks.  The buffers are only read, and may be reused when the call returns.  Host variables cross once per lane (num_variables x 32 bytes against 3 n x 32 of wires), device variables not at all.
 * The device copy of the map (3 n x 4 bytes), the variables staging of the single entry and, for the batches, one more lane group of
 * count x num_variables x 32 bytes -- it grows with the lanes and goes with them -- are counted in bbgpu_memory_info.staging_bytes and released with
 * the handle.  After a failure the handle stays usable and no MSM ticket is outstanding. */
int bbgpu_plonk_prover_set_witness_from(int prover, const bbgpu_plonk_witness* w);
int bbgpu_plonk_construct_proof_batch_from(int prover, int count, const bbgpu_plonk_witness* w /* count */, uint64_t* proofs_out);
int bbgpu_plonk_check_witness_batch_from(int prover, int count, const bbgpu_plonk_witness* w /* count */, bbgpu_plonk_witness_report* out /* count */);
int bbgpu_plonk_prover_destroy(int prover);
/* challenge.hpp:64-112 recomputed from a finished proof: gamma, beta, alpha, z (4 limbs each).  Host only, no GPU needed. */
int bbgpu_plonk_challenges_from_proof(const uint64_t proof[BBGPU_PLONK_PROOF_WORDS], uint64_t out[16]);

/* ---- host fallbacks of the drop-in boundary -----------------------------------------------------------------------
 * The reference API has no error channel (assert.hpp:13-23; batched_scalar_multiplications prints and returns, scalar_multiplication.cpp:680-684),
 * so a GPU call that fails at run time -- no device, an allocation refused on a shared GPU, a launch failure -- must not stop the prover:
 * shim/bb_shim.cpp logs the library's error once and computes the same result with these entries (csrc/host_fallback.hpp: textbook bucket
 * method / radix-2 transform / O(n) loops on the library's own host field code, a few host threads; never oracle/).  They make no HIP call,
 * take no lock and keep no state (re-entrant), accept what the GPU entries accept (any representative below 2^256) and return the same bytes
 * (canonical; MSM results normalised).  The GPU entries above never call them. */
int bbgpu_host_msm_g1(const uint64_t* scalars, const uint64_t* points, size_t n, int plain_table /* 0: 2n-entry endo table, 1: n-entry table */, uint64_t out[12]);
int bbgpu_host_ntt(uint64_t* coeffs, size_t n, int kind, const uint64_t* constant);
int bbgpu_host_fr_evaluate(const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t out[4]);
int bbgpu_host_kate_opening(const uint64_t* src, uint64_t* dest, size_t n, const uint64_t z[4], uint64_t f_of_z[4]);
int bbgpu_host_lagrange_l1_fft(uint64_t* l_1, size_t n_src, size_t n_target);
/* the host twins of the two entries on values (csrc/host_lagrange_open.hpp): plain loops with Montgomery's trick, the same argument verdict, host buffers
 * throughout; results are canonical field elements, so they equal the device entries' bit for bit.  No HIP call, no lock, re-entrant */
int bbgpu_host_fr_evaluate_lagrange(const uint64_t* values, size_t n, size_t stride_elems, int batch, const uint64_t z[4], uint64_t* out);
int bbgpu_host_kate_opening_lagrange(const uint64_t* values, uint64_t* quotient, size_t n, size_t stride_elems, int batch, const uint64_t z[4],
                                     uint64_t* f_of_z /* may be NULL */);
/* the twins of bbgpu_fr_fold_device and of a folded opening: plain loops (the fold, then the definition on the folded vector), the same argument verdicts;
 * stateless -- a session is a device-side economy, not part of the definition */
int bbgpu_host_fr_fold(uint64_t* out, const uint64_t* values, size_t n, size_t stride_elems, int batch, const uint64_t* gamma, int accumulate);
int bbgpu_host_kate_opening_lagrange_folded(const uint64_t* values, size_t n, size_t stride_elems, int batch, const uint64_t* gamma, const uint64_t z[4],
                                            uint64_t* quotient /* n */, int accumulate, uint64_t folded_f_of_z[4] /* may be NULL */);
int bbgpu_host_divide_by_pseudo_vanishing(uint64_t* coeffs, size_t n_src, size_t n_target);
/* bbgpu_plonk_check_witness on the host, for a caller without a GPU: the same definition, the same report; circuit->w_l / w_r / w_o are the witness.
 * Argument errors as bbgpu_plonk_prover_create (BBGPU_ERR_ARG: a null field, a widget's selectors given in part; BBGPU_ERR_SIZE: n). */
int bbgpu_host_plonk_check_witness(const bbgpu_plonk_circuit* circuit, bbgpu_plonk_witness_report* out);

/* ---- is this table an SRS?  (curve membership and the powers of x, checked on the GPU; the pairing on the host) ------
 * The entries above read, write, generate, cache and fingerprint structured reference strings and never ask whether the points are one:
 * bbgpu_transcript_read_g1 converts whatever 64-byte records the file holds, bbgpu_srs_register uploads them, and a row off the curve -- or a table
 * whose rows are not x^i G for the x behind the transcript's x G2 -- still yields BBGPU_OK and a proof the Verifier rejects two pairings later.
 * The reference pins the property for ONE pair of points (test/test_io.cpp:12-34, read_transcript_loads_well_formed_srs: e(-x G, G2) e(G, x G2) = 1,
 * plus g1::on_curve over the points); bbgpu_srs_check covers every row.
 * The pairing (curves/bn254/pairing.cpp over fields/field{2,6,12}.hpp, restated in csrc/host_pairing.hpp) is host code: these three entries make no
 * HIP call, take no lock and are re-entrant, like the bbgpu_host_* family. */
/* pairing::reduced_ate_pairing(P, Q) (pairing.cpp:333-347): out = 12 fq in the reference's fq12 order (c0.c0.c0, c0.c0.c1, c0.c1.c0 ... c1.c2.c1),
 * Montgomery, canonical.  p: affine G1 {x, y}, infinity flag honoured (result one).  q: g2::affine_element {x.c0, x.c1, y.c0, y.c1}, not infinity. */
int bbgpu_host_pairing(const uint64_t p[8], const uint64_t q[16], uint64_t out[48]);
/* is_one = (prod_k e(p_k, q_k) == 1) with one shared Miller-loop squaring chain and one final exponentiation (reduced_ate_pairing_batch,
 * pairing.cpp:364-385); p: k x 8 words, q: k x 16 words.  k == 0: one. */
int bbgpu_host_pairing_check(const uint64_t* p, const uint64_t* q, size_t k, int* is_one);
/* The check of k KZG openings (csrc/host_kzg_check.hpp), 1 <= k <= 64: claim t says that the polynomial committed to by C_t takes the value y_t at z_t, with
 * proof point pi_t (the commitment of the quotient, e.g. an MSM of what bbgpu_lagrange_opening_open_folded writes over a bbgpu_srs_lagrange handle).
 *   *ok = ( e(sum_t rho_t (C_t - y_t G + z_t pi_t), G2) e(-sum_t rho_t pi_t, x G2) == 1 ),  one pairing product of two pairs,
 * rho_t = bbgpu_srs_check's multipliers Keccak-256(seed, t) with the top three bits cleared, the seed rules the same (NULL: drawn from the operating
 * system).  commitments / proofs: k x 8 words, affine {x, y}, the infinity flag honoured; z / y: k x 4 words.  For a folded opening C_t is the caller's folded
 * commitment sum_b gamma_b C_b -- bbgpu_host_msm_g1 over a plain table of the commitments with gamma as it stands -- and y_t the folded value.
 * BBGPU_ERR_SIZE: k outside 1..64; BBGPU_ERR_ARG: a null pointer, a finite point off the curve, a g2_x that bbgpu_srs_check would not take.  Host only. */
int bbgpu_host_kzg_check_openings(const uint64_t* commitments /* k x 8 */, const uint64_t* z /* k x 4 */, const uint64_t* y /* k x 4 */,
                                  const uint64_t* proofs /* k x 8 */, size_t k, const uint64_t g2_x[16], const uint64_t seed[4] /* NULL: OS randomness */, int* ok);
/* the other half of io::read_transcript: the file's second G2 point, x * G2 (io.hpp:100-135,171-180), in Montgomery form */
int bbgpu_transcript_read_g2(const char* path, uint64_t g2_x_out[16]);

/* bbgpu_srs_check: rows [0, n) of a registered / generated table, P_i.
 *   curve test   every row satisfies y^2 = x^3 + 3 (one pass over the resident rows); row 0 is compared with the generator (1, 2)
 *   powers of x  with multipliers rho_i the table's maker could not know, A = sum_{i < n-1} rho_i P_i and B = sum_{i < n-1} rho_i P_{i+1} (two MSMs in
 *                flight over the same scalars, at offsets 0 and 1 of the handle) satisfy e(A, x G2) = e(B, G2) iff P_{i+1} = x P_i for every i, up to a
 *                soundness error of about 2^-253 per check.  Together with first_is_generator that is P_i = x^i G.
 * rho_i = Keccak-256(seed as 32 bytes, limbs little-endian || i as 8 bytes little-endian), the digest read as four little-endian 64-bit words with
 * the top three bits cleared (253 bits, below r), handed to the MSM as they are: the effective multipliers rho_i 2^-256 are uniform over 2^253 residues.
 * THE SEED MUST NOT BE KNOWN TO WHOEVER MADE THE TABLE -- a table can be built to pass for multipliers known in advance.  That is why seed == NULL
 * draws 32 bytes from the operating system (getrandom) and why the seed is reported only afterwards, so that a finding can be replayed.
 * Return codes: BBGPU_OK means the check RAN; the verdict is in the report.  A table is good iff bad_points == 0 and, when g2_x was given,
 * g2_ok && powers_ok.  BBGPU_ERR_ARG (unknown handle, n == 0, n beyond the table, null out, unknown flag bits) is refused before a device is bound.
 * The entry runs on context 0 under the library mutex; its scalars (n - 1 x 32 bytes) live in library staging counted in
 * bbgpu_memory_info.staging_bytes.  On any failure no MSM ticket is outstanding and the handle stays usable.  An honest table issues no atomic, and the
 * report does not vary from run to run; with the same seed it equals bbgpu_host_srs_check's field for field, a and b included.
 * BBGPU_SRS_CHECK_LOCATE: after a failed powers test the prefix length is bisected (prefix m passes iff every pair below m holds): at most ceil(log2 n)
 * more rounds of two MSMs and one pairing check, no new buffers.
 * Cost on one MI355X (tools/srs_check_bench.py, profiles/srs_check.txt; wall, one box): 2^16 rows 1.68 ms against 0.41 ms for the two MSMs alone, 2^20 rows 4.37 ms
 * against 2.81 ms; the excess (1.3 / 1.6 ms) is mostly the host tail (bbgpu_host_pairing_check of two pairs alone: 0.98 ms).  A negated row located: 22.8 / 48.4 ms.
 * The odd (endomorphism) entries of a caller's table are not validated: the library never reads them. */
typedef struct {
    uint64_t n;                 /* rows checked: points [0, n) of the handle */
    uint64_t bad_points;        /* rows with y^2 != x^3 + 3 */
    uint64_t first_bad_point;   /* smallest such row, UINT64_MAX if none */
    uint32_t first_is_generator;/* row 0 == (1, 2) */
    uint32_t g2_ok;             /* g2_x given, on the twist curve, not infinity, r * g2_x == infinity */
    uint32_t powers_checked;    /* the pairing test ran: g2_ok && bad_points == 0 && n >= 2 */
    uint32_t powers_ok;         /* e(A, x G2) == e(B, G2) */
    uint64_t first_bad_power;   /* with BBGPU_SRS_CHECK_LOCATE and !powers_ok: smallest i with P_{i+1} != x P_i, else UINT64_MAX */
    uint64_t seed[4];           /* the seed used (the caller's, or the one drawn), so that a finding can be replayed */
    uint64_t a[8], b[8];        /* A = sum_{i<n-1} rho_i P_i,  B = sum_{i<n-1} rho_i P_{i+1}, affine (infinity flag honoured; infinity when the test did not run) */
} bbgpu_srs_report;
#define BBGPU_SRS_CHECK_LOCATE 1
int bbgpu_srs_check(int srs_handle, size_t n, const uint64_t g2_x[16] /* NULL: curve test only */, const uint64_t seed[4] /* NULL: OS randomness */,
                    int flags, bbgpu_srs_report* out);
/* the same definition over the even entries of a caller's 2n-entry endo table, on the host (csrc/host_srs_check.hpp: a plain loop for the curve test,
 * the bucket method behind bbgpu_host_msm_g1 for A and B, the same pairing tail and bisection); no HIP call, no lock */
int bbgpu_host_srs_check(const uint64_t* points_endo_table, size_t n, const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_srs_report* out);

/* ---- make this SRS your own: rows times powers of a secret, with proof ------
 * A universal, updatable string is one anybody may multiply a secret of their own into: from P_i = x^i G and x G2 to (x y)^i G and (x y) G2, after which
 * the string is sound as long as ONE contributor's secret is forgotten.  bbgpu_srs_update is that operation on a resident table, row-wise:
 *   row i  <-  y^(first_power + i) * P_i                     n independent variable-base multiplications by 254-bit scalars
 * and bbgpu_host_srs_update_check is the proof a third party needs that the new string is the old one with some secret multiplied in.
 * The reference has no counterpart (its strings come from a file, io.hpp:159-181).
 *   y            Montgomery form, any representative below 2^256.  y == 0 (mod r) is refused (BBGPU_ERR_ARG: every row would be infinity); y == 1 copies.
 *   first_power  exists so that a point-range share of a larger string (bbgpu_srs_generate_range) is updated with the powers it owns; first_power + n <= 2^32.
 *   bad rows     the resident form has no infinity row and a point off the curve has no defined multiple: the curve pass of bbgpu_srs_check (k_srs_on_curve)
 *                runs over the input rows first; if any fails, the report is written (when out is given), NO table is made and the entry returns
 *                BBGPU_ERR_ARG, bbgpu_last_error() naming the first bad row.
 *   new table    a NEW resident table, added the way bbgpu_srs_generate_range adds its own: window tables under the same conditions (bbgpu_set_precompute,
 *                n >= 1024; an allocation the tables cannot get is ridden out without them, as there), host_endo_table_out -- filled by the export kernel of
 *                bbgpu_srs_generate -- as the address key when given.  The input handle is untouched and stays valid.
 *   G2 half      host work: y_g2 = y G2 and g2_x_out = y * g2_x by the double-and-add of bbgpu_transcript_write.  Only the FIRST power enters G2, whatever
 *                first_power: e(P_{i+1}, G2) = e(P_i, x y G2) for every consecutive pair of rows.
 * Return codes: the new handle (>= 0), or BBGPU_ERR_ARG (unknown handle, n == 0, n beyond the table, null y_mont, y == 0 mod r, first_power + n > 2^32 --
 * all refused before a device is bound -- or a row off the curve), or BBGPU_ERR_HIP.  On any failure no handle has been created, nothing the call allocated
 * is still live and no MSM ticket is outstanding.  The entry runs on context 0 under the library mutex; every allocation, copy and launch check passes the
 * fault-injection funnels (a warm call: 1-2 allocations + those of the window tables, one upload, one read-back + the host table's, 2-3 launch checks + one per
 * window-table segment).
 * The kernel (csrc/srs_update.hip, k_srs_update): one lane per row; s = y^(first_power + i) in Fr, k = its plain value, k = k1 - lambda k2 with both halves
 * below 2^128 (the split of fr::split_into_endomorphism_scalars with the sign of k2 kept, so that it holds for EVERY k), then one ladder over both halves
 * with 3-bit windows of odd signed digits on P and on (beta x, -y) = -lambda P: 126 doublings and 88 complete additions, a Fermat inversion per row.
 * With bbgpu_set_timing(1), bbgpu_last_timing() index 0 is the device time of k_srs_update alone (a pair of events around it).
 * Cost on one MI355X (tools/srs_update_bench.py, profiles/srs_update.txt; wall, one box): 2^16 rows 5.33 ms, 7.18 ms with the host table, 1.91 ms when the
 * new handle gets no window tables (bbgpu_set_precompute(0)); 2^20 rows 56.1 / 78.9 / 17.1 ms.  k_srs_update alone 1.21 ms and 16.4 ms (15.7 ns per row,
 * ~2850 field products per row: 182 G products/s with squarings counted as products); the rest of a 2^20 call is the window tables of the new handle (39 ms)
 * and the host table's export and read-back (15-23 ms).  The G2 half is 0.65 ms of host time whatever n.  Host twin: 22 ms per 4096 rows on 16 threads.
 * The host twin (csrc/host_srs_update.hpp) is a plain double-and-add per row on a few threads; the results are unique affine points, so the two agree bit
 * for bit, reports included.  bbgpu_host_srs_update, bbgpu_host_srs_update_check and bbgpu_transcript_write_g2 make no HIP call, take no lock and are
 * re-entrant, like the bbgpu_host_* family. */
typedef struct {
    uint64_t n;                /* rows written */
    uint64_t first_power;      /* row i was multiplied by y^(first_power + i) */
    uint64_t bad_points;       /* input rows off the curve (no table is made when > 0) */
    uint64_t first_bad_point;  /* smallest such row, UINT64_MAX if none */
    uint32_t g2_ok;            /* g2_x given and valid as bbgpu_srs_check judges it */
    uint32_t _pad;
    uint64_t y_g2[16];         /* y * G2: the public half of the update, for bbgpu_host_srs_update_check */
    uint64_t g2_x_out[16];     /* y^1 * g2_x when g2_ok, else zero: the x G2 of the updated string */
} bbgpu_srs_update_report;
/* rows [0, n) of a registered / generated table -> a NEW resident table, row i = y^(first_power + i) * P_i; returns its handle >= 0 */
int bbgpu_srs_update(int srs_handle, size_t n, size_t first_power, const uint64_t y_mont[4], const uint64_t g2_x[16] /* NULL: no G2 half */,
                     uint64_t* host_endo_table_out /* NULL: resident only */, bbgpu_srs_update_report* out /* may be NULL */);
/* the same over the even entries of a caller's 2n-entry endo table, on the host; writes all 2n entries of table_out (may alias points_endo_table).
 * A row off the curve: the report, BBGPU_ERR_ARG and an untouched table_out. */
int bbgpu_host_srs_update(const uint64_t* points_endo_table, size_t n, size_t first_power, const uint64_t y_mont[4], const uint64_t g2_x[16],
                          uint64_t* table_out, bbgpu_srs_update_report* out /* may be NULL */);
/* is `new` the string `old` with its secret multiplied by the discrete log of y_g2?  *ok = y_g2 on the twist, finite, of order r AND
 * e(old_p1, y_g2) e(-new_p1, G2) == 1 (one bbgpu_host_pairing_check of two pairs).  old_p1 / new_p1: row 1 of either table, affine {x, y}.  Together with
 * bbgpu_srs_check of the new table against its g2_x_out this covers every row: the check says the rows are powers of ONE secret, this says which. */
int bbgpu_host_srs_update_check(const uint64_t old_p1[8], const uint64_t new_p1[8], const uint64_t y_g2[16], int* ok);
/* bbgpu_transcript_write for a string whose secret nobody holds: the caller gives x G2 itself (BBGPU_ERR_ARG unless bbgpu_srs_check would accept it) */
int bbgpu_transcript_write_g2(const char* path, const uint64_t* points_endo_table, size_t degree, const uint64_t g2_x[16]);

/* ---- the same string in the Lagrange basis: a group inverse NTT of a resident table ------
 * Every table above is in the monomial basis, P_j = x^j G.  A caller who holds a polynomial as its VALUES v_i on the size-n domain commits to it over
 *   L_i = n^-1 * sum_{j<n} omega^(-i j) * P_j          (for an honest string this is L_i(x) G; omega the root the transforms use, fr_root_of_unity(log2 n))
 * without an inverse transform first: with c = ifft(v), sum_i v_i L_i = sum_j c_j P_j.  bbgpu_srs_lagrange makes that table from rows [0, n) of a resident
 * one: an inverse NTT whose elements are curve points, n/2 log2 n variable-base multiplications by 254-bit twiddles.  The reference has no counterpart.
 *   n            a power of two, 2 <= n <= 2^22, no larger than the table: otherwise BBGPU_ERR_SIZE.  n == 0 or an unknown handle: BBGPU_ERR_ARG.  All of
 *                these are refused before a device is bound.
 *   bad rows     as in bbgpu_srs_update: the curve pass (k_srs_on_curve) runs over the input rows first; if any fails, the report is written (when out is
 *                given), NO table is made and the entry returns BBGPU_ERR_ARG, bbgpu_last_error() naming the first bad row.
 *   infinity     the resident form has no infinity row, so an OUTPUT row at infinity is refused the same way: infinity_rows and first_infinity_row in the
 *                report, BBGPU_ERR_ARG, the message naming the first such row, no table.  (The table of x = omega^k has L_i = delta_ik G.)  Infinities and
 *                doublings INSIDE the transform are no errors: every addition is complete.
 *   new table    a NEW resident table, added the way bbgpu_srs_update adds its own: window tables under the same conditions (bbgpu_set_precompute,
 *                n >= 1024; an allocation the tables cannot get is ridden out without them), host_endo_table_out -- filled by the export kernel of
 *                bbgpu_srs_generate -- as the address key when given.  The input handle is untouched and stays valid; every MSM entry serves the new one.
 * Return codes: the new handle (>= 0), BBGPU_ERR_SIZE, BBGPU_ERR_ARG or BBGPU_ERR_HIP.  On any failure no handle has been created, nothing the call
 * allocated is still live and no MSM ticket is outstanding.  The entry runs on context 0 under the library mutex; every allocation, copy and launch check
 * passes the fault-injection funnels (a warm call: the scratch and the new rows + the export buffer + those of the window tables; one upload; two
 * read-backs + the host table's; two launch checks -- the curve pass, and the chain of load, stage and finish kernels -- + the export kernel's + one per
 * window-table segment).
 * The kernels (csrc/srs_lagrange.hip): radix-2, decimation in time, on a scratch of n projective points (XYZZ, 128 bytes each, ZZ == 0 for infinity).
 * k_lagrange_load puts n^-1 * P_bitrev(i) into slot i (one ladder per row); log2 n launches of k_lagrange_stage (csrc/g1_stage.hpp) run (a, b) -> (a + w b, a - w b) in place,
 * one lane per butterfly, w = omega^-e made in the lane by square-and-multiply and w b by the ladder of k_srs_update (csrc/g1_ladder.hpp: signed
 * endomorphism split, 3-bit odd signed windows, 126 doublings) over a projective base and without its inversion -- butterflies with w = 1 skip it;
 * k_lagrange_finish normalises with one Fermat inversion per row and counts the rows at infinity.
 * With bbgpu_set_timing(1), bbgpu_last_timing() index 0 is the device time of the stage kernels alone, index 1 that of k_lagrange_load, index 2 that of
 * k_lagrange_finish.
 * Cost on one MI355X (tools/srs_lagrange_bench.py, profiles/srs_lagrange.txt; one box, k_srs_update measured in the same run): 2^20 rows 183.8 ms wall,
 * 204.5 ms with the host table, 145.8 ms when the new handle gets no window tables; the stage kernels alone 129.6 ms = 13.7 ns per butterfly that runs a
 * ladder (~2520 field products; k_srs_update in that run: 15.4 ns per row), the load kernel 14.2 ms, the finish kernel 1.9 ms.  2^16 rows 19.6 ms wall
 * (stages 14.7 ms), 2^12 rows 17.4 ms (stages 10.7 ms): below 2^18 rows a stage launch no longer fills the chip and every stage costs the ~0.9 ms one wave
 * needs for its ladder, so small conversions cost log2 n x 0.9 ms.  Host twin: 107 ms per 4096 rows on 16 threads.
 * The host twin (csrc/host_srs_lagrange.hpp) is a plain radix-2 over host_g1.hpp with a plain double-and-add per twiddle on a few threads; the results are
 * unique affine points, so the two agree bit for bit, reports included.  It makes no HIP call, takes no lock and is re-entrant. */
typedef struct {
    uint64_t n;                  /* rows converted: rows [0, n) of the handle */
    uint64_t bad_points;         /* input rows off the curve (no table is made when > 0) */
    uint64_t first_bad_point;    /* UINT64_MAX if none */
    uint64_t infinity_rows;      /* OUTPUT rows that are the point at infinity (no table is made when > 0) */
    uint64_t first_infinity_row; /* UINT64_MAX if none */
} bbgpu_srs_lagrange_report;
/* rows [0, n) of a registered / generated table -> a NEW resident table, row i = L_i; returns its handle >= 0 */
int bbgpu_srs_lagrange(int srs_handle, size_t n, uint64_t* host_endo_table_out /* NULL: resident only */, bbgpu_srs_lagrange_report* out /* may be NULL */);
/* the same over the even entries of a caller's 2n-entry endo table, on the host; writes all 2n entries of table_out (may alias points_endo_table).
 * A row off the curve or an output row at infinity: the report, BBGPU_ERR_ARG and an untouched table_out. */
int bbgpu_host_srs_lagrange(const uint64_t* points_endo_table, size_t n, uint64_t* table_out /* 2n entries, may alias */,
                            bbgpu_srs_lagrange_report* out /* may be NULL */);

/* ---- is this table the Lagrange form of that string?  (two MSMs and one transform; no pairing) ------
 * bbgpu_srs_lagrange is expensive, so its table is made once, exported (host_endo_table_out) and registered again in later runs -- after which nothing
 * above can say whether the registered rows R_i still are the L_i of the string: bbgpu_srs_check fails such a table by construction (its rows are not powers
 * of x), and a wrong row yields BBGPU_OK and a commitment the verifier rejects.  bbgpu_srs_lagrange_check answers it for rows [0, n) of both handles:
 *   curve test   every row of the Lagrange table satisfies y^2 = x^3 + 3 (the pass of bbgpu_srs_check; row 0 is not compared with the generator)
 *   basis test   with the multipliers rho_i of bbgpu_srs_check (same derivation from the seed, same seed rules, i < n), A = sum_i rho_i R_i over the
 *                Lagrange handle and B = sum_j ifft(rho)_j P_j over the monomial handle (a copy of rho transformed in place by BBGPU_IFFT; two MSM
 *                tickets in flight) are the same point iff R_i = L_i for every i, up to a soundness error of about 2^-253: B = sum_i rho_i L_i, and a
 *                non-zero combination of the differences R_i - L_i vanishes at random multipliers with that chance.  The two normalised points are
 *                compared on the host.
 * Whether the monomial string itself is honest is bbgpu_srs_check's question, not this entry's.
 * BBGPU_SRS_LAGRANGE_CHECK_LOCATE: after a failed basis test the prefix length m is bisected -- A over the first m multipliers and rows, B over the
 * transform of rho with the entries from m on zeroed; prefix m passes iff every row below m is right -- at most ceil(log2 n) more rounds of one transform
 * and two MSMs, no buffer beyond the copy.
 * Return codes: BBGPU_OK means the check RAN; the verdict is in the report (good iff bad_points == 0 && basis_ok).  BBGPU_ERR_SIZE: n not a power of two
 * in [2, 2^22] or larger than either table.  BBGPU_ERR_ARG: an unknown handle, null out, unknown flag bits.  All are refused before a device is bound.
 * The entry runs on context 0 under the library mutex; the multipliers and their copy (2 n x 32 bytes) live in the staging of bbgpu_srs_check, counted in
 * bbgpu_memory_info.staging_bytes.  After any failure no MSM ticket is outstanding and both handles stay usable; neither table is written.  With the same
 * seed the report equals bbgpu_host_srs_lagrange_check's field for field, a and b included.  A warm honest check of 4096 rows without LOCATE passes no
 * allocation, one upload, one read-back and six launch checks (the curve pass, the multipliers, the transform's two passes, one per MSM) and
 * synchronises twice before the tickets are issued (the curve verdict, the transformed copy).
 * Cost on one MI355X (tools/lagrange_open_bench.py, profiles/lagrange_open.txt; wall, one box): 2^16 rows 0.479 ms against 0.381 ms for two device MSMs in
 * flight over the same handles alone, 2^20 rows 2.965 against 2.580 ms: the check costs its two MSMs plus 0.10 / 0.39 ms for the curve pass, the
 * multipliers, the copy, the transform and the two synchronisations; no pairing, so no host tail. */
#define BBGPU_SRS_LAGRANGE_CHECK_LOCATE 1
typedef struct {
    uint64_t n;                 /* rows checked: rows [0, n) of both handles */
    uint64_t bad_points;        /* rows of the Lagrange table off the curve */
    uint64_t first_bad_point;   /* smallest such row, UINT64_MAX if none */
    uint32_t basis_checked;     /* the basis test ran: bad_points == 0 */
    uint32_t basis_ok;          /* sum_i rho_i R_i == sum_j ifft(rho)_j P_j */
    uint64_t first_bad_row;     /* with BBGPU_SRS_LAGRANGE_CHECK_LOCATE and !basis_ok: smallest i whose row is not L_i, else UINT64_MAX */
    uint64_t seed[4];           /* the seed used (the caller's, or the one drawn), so that a finding can be replayed */
    uint64_t a[8], b[8];        /* the two sums, affine (infinity flag honoured; infinity when the test did not run) */
} bbgpu_srs_lagrange_check_report;
int bbgpu_srs_lagrange_check(int lagrange_handle, int monomial_handle, size_t n, const uint64_t seed[4] /* NULL: OS randomness */, int flags,
                             bbgpu_srs_lagrange_check_report* out);
/* the same definition over the even entries of two 2n-entry endo tables, on the host (csrc/host_srs_lagrange_check.hpp: the curve loop, the transform and
 * the bucket method of the bbgpu_host_* family, the same verdict and bisection); no HIP call, no lock */
int bbgpu_host_srs_lagrange_check(const uint64_t* lagrange_endo_table, const uint64_t* monomial_endo_table, size_t n, const uint64_t seed[4], int flags,
                                  bbgpu_srs_lagrange_check_report* out);

/* ---- open a polynomial at every point of its domain: all n KZG proofs at once ------
 * The opening proof of f = sum_j c_j X^j at z is pi(z) = [(f(X) - f(z)) / (X - z)](x) G = sum_{m <= n-2} z^m h_m with h_m = sum_{j > m} c_j P_(j-m-1).  Every
 * entry above prices one proof at an O(n) quotient pass and an n-point MSM; a caller who needs the proof at EVERY point of the size-n domain (data
 * availability sampling, vector commitments, lookup tables, one evaluation with its proof per party) would pay that n times.  The n proofs are one
 * structured linear map of the string (Feist and Khovratovich): (pi(omega^0) .. pi(omega^(n-1))) is the forward size-n group transform of
 * (h_0 .. h_(n-2), infinity), and h is a Toeplitz product that one cyclic convolution of length N = 2 n delivers.  With omega = fr_root_of_unity(log2 n) and
 * W = fr_root_of_unity(log2 n + 1), the roots the transforms and bbgpu_srs_lagrange use:
 *   s = (P_(n-2), P_(n-3), .., P_0, infinity x (n + 1))        the string only
 *   t = (c_(n-1), 0 x (n + 1), c_1, c_2, .., c_(n-2))          (n = 2: (c_1, 0, 0, 0))
 *   h = the first n entries of IDFT_N(DFT_N(s) o DFT_N(t)), root W, the product pointwise
 * O(n log n) group operations in place of n MSMs.  The reference has no counterpart.
 * bbgpu_kzg_open_all_setup computes S^ = DFT_N(s) ONCE from rows [0, n - 1) of a resident monomial table and keeps its N rows on the device (scratch form,
 * 128 bytes each, ZZ == 0 for infinity; counted in bbgpu_memory_info.staging_bytes, released by bbgpu_kzg_open_all_release or bbgpu_shutdown).
 *   n            a power of two, 2 <= n <= 2^21, no larger than the table: otherwise BBGPU_ERR_SIZE.  An unknown SRS handle: BBGPU_ERR_ARG.
 *                BBGPU_ERR_STATE: BBGPU_KZG_OPEN_ALL_MAX_SETUPS setups are live.  All are refused before a device is bound.
 *   bad rows     the curve pass (k_srs_on_curve) runs over the input rows first, as in bbgpu_srs_lagrange: a bad row is BBGPU_ERR_ARG, bbgpu_last_error()
 *                naming the first one, and no setup is made.
 *   infinity     a row of S^ at infinity is legal and kept exactly -- it is an intermediate, not a table anyone commits over.  It happens when
 *                (W^k / x)^(n-1) = 1 and W^k != x; at n = 4 that is x = W^k zeta, zeta a primitive cube root of unity in Fr.
 * Returns the setup handle (>= 0).  A warm setup passes one allocation (S^), one upload and one read-back (the curve findings) and two launch checks (the
 * curve pass; the chain of k_open_cosets_string and the log2 N stage kernels).  The SRS handle is not read after the setup returns and may be released.
 * bbgpu_kzg_open_all_device opens `batch` polynomials in coefficient form over one setup: coefficient j of polynomial b at
 * d_coeffs[(b * stride_elems + j) * 4] (device memory, read only; the reference's memory format, any representative), and writes batch x n affine points to
 * HOST memory: proofs_out[(b * n + i) * 8] is pi_b(omega^i) in the reference's format (Montgomery-256, canonical; infinity: bit 63 of y[3], every other word
 * zero).  Infinity is an ordinary result: a constant polynomial has every proof at infinity.  The evaluations y_i = f(omega^i) are one bbgpu_ntt_device
 * away for the caller; this entry does not return them.
 *   BBGPU_ERR_SIZE   batch outside 1..64, stride_elems < n, batch x 2 n > 2^22
 *   BBGPU_ERR_ARG    an unknown setup, a null pointer                                    -- all refused before a device is bound
 * The kernels are those of bbgpu_kzg_open_cosets_device (the next block) at coset size 1 without a degree bound: a setup of this block is such a setup, kept
 * in a pool of its own (csrc/kzg_open_cosets.hip; every one takes the polynomial from blockIdx.y, so that a batch of small domains fills the chip):
 * k_open_cosets_t writes the batch x N scalars of t and bbgpu_ntt_device_batch transforms them; k_open_cosets_sum, which at this size adds nothing, puts
 * (N^-1 t^_bitrev(i)) * S^_bitrev(i) into slot i -- each lane reads its own scalar, brings it to a plain canonical integer by one product and runs one ladder (csrc/g1_ladder.hpp) over a projective base; a zero scalar or
 * an infinite base gives infinity; log2 N launches of k_lagrange_stage (csrc/g1_stage.hpp, the one text bbgpu_srs_lagrange launches too) with root W^-1;
 * k_open_cosets_gather copies slots 0 .. n-2 bit-reversed into the upper half of the polynomial's own slots, with infinity last; log2 n launches of
 * k_lagrange_stage with root omega there; k_open_cosets_finish normalises with one Fermat inversion per row and refuses nothing.  One wave per workgroup,
 * 3-bit windows, no twiddle table, as bbgpu_srs_lagrange.
 * The entry runs on context 0 under the library mutex; every allocation, copy and launch check passes the fault-injection funnels.  A warm call at n = 64:
 * two allocations (t, which later holds the proofs, and the scratch points), no upload, one read-back (the proofs: one staging chunk), and three launch
 * checks (k_open_cosets_t; the transform's single pass at this size; the chain from the sum kernel to the finish kernel).  After a failure nothing the call allocated is live and
 * the setup stays usable.  With bbgpu_set_timing(1), bbgpu_last_timing() index 0 is the device time of k_open_cosets_sum, 1 that of the inverse stages, 2 that
 * of the gather kernel and the forward stages, 3 that of k_open_cosets_finish.
 * Cost on one MI355X (tools/kzg_open_all_bench.py, profiles/kzg_open_all.txt): wall ms per call, proofs read back to the host, one box.  n = 2^12:
 * 24.5 ms at batch 1 and 28.0 ms at batch 16 -- a single 4096-row call is bound by the latency of its 25 stage launches (the inverse stages 12.1 ms, the
 * gather and the forward stages 11.1 ms, the kernel of the ladders (then k_open_all_load, a kernel of this entry's own) 1.0 ms, the finish kernel 0.15 ms of device time), and fifteen more polynomials ride along for
 * 3.6 ms; n = 2^16: 34.8 ms at batch 1, 348 ms at batch 16 (the chip is full: inverse stages 214 ms, forward 102 ms, load 28 ms); n = 2^20: 433 ms (inverse
 * stages 271 ms = 12.9 ns per butterfly that runs a ladder, forward 130 ms, load 28 ms, finish 1.9 ms).  The setup, with its release: 12.2 ms, 16.8 ms and
 * 271 ms.  Against the path a caller had before -- bbgpu_kate_opening_device, then bbgpu_msm_g1_device, per point over the same handle, timed in the same
 * process on a SAMPLE of 256 points and SCALED to all n (an extrapolation): 1.54 s at 2^12, 24.2 s at 2^16 and 1487 s at 2^20 per polynomial; the new
 * entry is lower at every size measured, by far more than either spread.
 * The host twin (that of the next block at coset size 1, csrc/host_kzg_open_cosets.hpp) runs the same construction over host_g1.hpp: the scalar transform of the bbgpu_host_* family, the radix-2
 * group transform of bbgpu_host_srs_lagrange and a plain double-and-add per product.  The results are unique affine points, so device and twin agree bit
 * for bit.  It takes the even entries of a caller's endo table (at least n - 1 rows are read), makes no HIP call, takes no lock and is re-entrant; its
 * errors are those of the two device entries (a row off the curve: BBGPU_ERR_ARG naming it). */
#define BBGPU_KZG_OPEN_ALL_MAX_SETUPS 16
int bbgpu_kzg_open_all_setup(int srs_handle, size_t n); /* setup handle >= 0 */
int bbgpu_kzg_open_all_release(int setup);
int bbgpu_kzg_open_all_device(int setup, const uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* proofs_out /* host, batch x n x 8 */,
                              void* hip_stream);
int bbgpu_host_kzg_open_all(const uint64_t* points_endo_table, size_t n, const uint64_t* coeffs, size_t stride_elems, int batch,
                            uint64_t* proofs_out /* batch x n x 8 */);

/* ---- open a polynomial on every coset of its domain: all n / l KZG cell proofs at once ------
 * A data-availability sampler does not ship one proof per point but CELLS: the l evaluations on one coset of the domain with ONE proof for all l of them
 * (the multi-proofs of the same paper of Feist and Khovratovich).  With l = `coset` a power of two, m = n / l >= 2, omega = fr_root_of_unity(log2 n) and
 * psi = omega^l = fr_root_of_unity(log2 m): coset k < m is { omega^(k + m j) : j < l }, its vanishing polynomial is X^l - psi^k, and
 *   pi_k = [q_k(x)] G,  f = q_k (X^l - psi^k) + r_k,  deg r_k < l.
 * (pi_0 .. pi_(m-1)) is the forward size-m group transform, root psi, of (h_0 .. h_(m-2), infinity) with h_u = sum_{j >= (u+1) l} c_j P_(j - (u+1) l).
 * Split by residue e = j mod l, c^(e)_a = c_(e + l a) and P^(e)_b = P_(e + l b): h = sum_e Toeplitz(c^(e), P^(e)), each term in the layout of the block
 * above at size m.  With M = 2 m and W = fr_root_of_unity(log2 M):
 *   s^(e) = (P^(e)_(m-2), .., P^(e)_0, infinity x (m + 1))
 *   t^(e) = (c^(e)_(m-1), 0 x (m + 1), c^(e)_1, .., c^(e)_(m-2))          (m = 2: (c^(e)_1, 0, 0, 0))
 *   h = the first m entries of IDFT_M( sum_e DFT_M(s^(e)) o DFT_M(t^(e)) )
 * The l products are summed in the Fourier domain, so ONE inverse transform of length M and ONE forward transform of length m serve all l residues: the
 * 2 n ladder products of bbgpu_kzg_open_all_device, and l times fewer group butterflies.  A caller of that entry gets the same proofs by folding l single
 * proofs per cell on the host: pi_k = sum_j [omega^(k + m j) / (l psi^k)] pi(omega^(k + m j)); the tests tie the two entries by that identity.  The
 * reference has no counterpart.
 * bbgpu_kzg_open_cosets_setup computes S^(e) = DFT_M(s^(e)) for every e < l ONCE from rows [0, n - l) of a resident monomial table and keeps the l x M =
 * 2 n rows on the device (the footprint of an open-all setup; counted in bbgpu_memory_info.staging_bytes, released by bbgpu_kzg_open_cosets_release or
 * bbgpu_shutdown).
 *   n, coset     powers of two, 1 <= coset <= BBGPU_KZG_OPEN_COSETS_MAX_COSET, n / coset >= 2, n <= 2^21 and no larger than the table: otherwise
 *                BBGPU_ERR_SIZE.  An unknown SRS handle: BBGPU_ERR_ARG.  BBGPU_ERR_STATE: BBGPU_KZG_OPEN_COSETS_MAX_SETUPS setups are live -- a pool of its
 *                own: the setups of bbgpu_kzg_open_all_setup neither count against it nor are refused by it (those of bbgpu_kzg_open_cosets_setup_bounded,
 *                the next block, are setups of this pool).  All are refused before a device is bound.
 *   coset == 1   is accepted on purpose: the construction is then that of the block above, and the proofs are those of bbgpu_kzg_open_all_device bit for bit.
 *   bad rows     the curve pass runs over the rows the setup reads, [0, n - l), as in bbgpu_kzg_open_all_setup: a bad row is BBGPU_ERR_ARG,
 *                bbgpu_last_error() naming the first one, and no setup is made.  Rows from n - l on are not read.
 *   infinity     a row of S^(e) at infinity is legal and kept exactly.
 * Returns the setup handle (>= 0).  A warm setup passes one allocation (S^), one upload and one read-back (the curve findings) and two launch checks (the
 * curve pass; the chain of k_open_cosets_string and the log2 M stage kernels).  The SRS handle is not read after the setup returns and may be released.
 * bbgpu_kzg_open_cosets_device opens `batch` polynomials in coefficient form over one setup: coefficient j of polynomial b at
 * d_coeffs[(b * stride_elems + j) * 4] (device memory, read only; the reference's memory format, any representative), and writes batch x m affine points to
 * HOST memory: proofs_out[(b * m + k) * 8] is pi_k of polynomial b in the reference's format (Montgomery-256, canonical; infinity: bit 63 of y[3], every
 * other word zero).  Infinity is an ordinary result: a polynomial of degree below l has every proof at infinity.  The order is natural in k: the values of
 * cell k are entries k, k + m, k + 2 m, .. of the caller's own size-n bbgpu_ntt_device of the coefficients; this entry does not return them.
 *   BBGPU_ERR_SIZE   batch outside 1..64, stride_elems < n (< d over a setup with a degree bound d: the next block), batch x 2 n > 2^22
 *   BBGPU_ERR_ARG    an unknown setup, a null pointer                                    -- all refused before a device is bound
 * The kernels (csrc/kzg_open_cosets.hip; every one takes the polynomial from blockIdx.y): k_open_cosets_t writes the batch x l x M scalars of t^(e) and
 * bbgpu_ntt_device_batch transforms them, 64 transforms per call; k_open_cosets_sum puts sum_e (M^-1 t^^(e)_j) * S^(e)_j, j = bitrev(i), into slot i --
 * one wave takes 64 / l frequencies, lane (f, e) brings its own scalar to a plain integer and runs one ladder (csrc/g1_ladder.hpp) over its own projective
 * base, and the l results of a frequency are added in a log2 l-level tree across lanes, the points crossing in 8 KiB of LDS; the additions are complete
 * (either side at infinity, equal points, opposite points); log2 M launches of k_lagrange_stage (csrc/g1_stage.hpp) with root W^-1; k_open_cosets_gather,
 * log2 m launches of k_lagrange_stage with root psi and k_open_cosets_finish work as the block above says, at sizes m and M.
 * The entry runs on context 0 under the library mutex; every allocation, copy and launch check passes the fault-injection funnels.  A warm call at
 * (n, l) = (256, 4): two allocations (t, which later holds the proofs, and the scratch points), no upload, one read-back (the proofs: one staging chunk),
 * and three launch checks (k_open_cosets_t; the transform's single pass at this size -- one more for every further group of 64 transforms; the chain from
 * the sum kernel to the finish kernel).  After a failure nothing the call allocated is live and the setup stays usable.  With bbgpu_set_timing(1),
 * bbgpu_last_timing() index 0 is the device time of k_open_cosets_sum, 1 that of the inverse stages, 2 that of the gather kernel and the forward stages,
 * 3 that of k_open_cosets_finish.
 * Cost on one MI355X (tools/kzg_open_cosets_bench.py, profiles/kzg_open_cosets.txt): wall ms per call, proofs read back to the host, one box, against
 * bbgpu_kzg_open_all_device at the same n and batch TIMED IN THE SAME PROCESS in alternating pairs -- the n single proofs only: the l-point host fold per
 * cell that the old path needs on top was not timed and is not charged.  l = 64: n = 2^12 13.2 ms against 24.5 (batch 16: 15.9 against 26.9); n = 2^16
 * 21.7 against 35.0 (batch 16: 50.1 against 351); n = 2^20 57.4 against 436 (medians of 3 pairs; the others of 9).  l = 4 at n = 2^16: 30.1 against 34.9
 * (batch 16: 104 against 349).  The new entry is lower in every cell, by more than the full range (max - min) of either leg's timings.  Device times at
 * (2^20, 64): the sum kernel 31.4 ms, the inverse stages 14.0 ms, the gather and the forward stages 13.1 ms, the finish kernel 0.16 ms -- the 2 n ladders
 * are now more than half the call, and a call of few polynomials stays bound from below by the latency of its log2 M + log2 m stage launches (about 0.9
 * ms each: 12.0 of 13.2 ms at (2^12, 64)).  k_open_cosets_sum against k_open_all_load, the treeless kernel the open-all entries then had, over the same 2 n ladders, both from bbgpu_set_timing in that
 * process:
 * +0.96 ms on 30.4 at 2^20 and +0.15 on 2.2 at 2^16 -- the tree and the LDS crossing cost 3 to 7 percent of the kernel.  231 VGPRs against 229, no scratch
 * memory in either (the compiler's resource remarks, at the head of the profile).  The setup, with its release: 6.5 ms, 10.8 ms and 187 ms at l = 64, 14.7
 * ms at (2^16, 4).  Nothing was tuned after these measurements.
 * The host twin (csrc/host_kzg_open_cosets.hpp) runs the same construction over host_g1.hpp with a plain double-and-add per product and a plain
 * left-to-right sum over e.  The results are unique affine points, so device and twin agree bit for bit.  It takes the even entries of a caller's endo
 * table (n - l rows are read), makes no HIP call, takes no lock and is re-entrant; its errors are those of the two device entries (a row off the curve:
 * BBGPU_ERR_ARG naming it). */
#define BBGPU_KZG_OPEN_COSETS_MAX_SETUPS 16
#define BBGPU_KZG_OPEN_COSETS_MAX_COSET 64
int bbgpu_kzg_open_cosets_setup(int srs_handle, size_t n, size_t coset); /* setup handle >= 0 */
int bbgpu_kzg_open_cosets_release(int setup);
int bbgpu_kzg_open_cosets_device(int setup, const uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* proofs_out /* host, batch x (n / coset) x 8 */,
                                 void* hip_stream);
int bbgpu_host_kzg_open_cosets(const uint64_t* points_endo_table, size_t n, size_t coset, const uint64_t* coeffs, size_t stride_elems, int batch,
                               uint64_t* proofs_out /* batch x (n / coset) x 8 */);

/* ---- open cosets of a polynomial of BOUNDED DEGREE: half the ladders at d = n / 2, and a string of d rows is enough ------
 * Everything downstream of the block above is built around a polynomial of degree < d on a domain of size n > d (bbgpu_kzg_recover_cells wants
 * count x l >= d, bbgpu_g1_recover extends k rows to 2 k), but a setup of the block above treats every polynomial as degree < n: n - l rows of the string,
 * 2 n rows of S^, 2 n ladders and an inverse transform of length 2 n / l per call.  For degree < d = `degree_bound` the Toeplitz products of the same
 * construction have size mu = d / l, not m = n / l; only the last forward transform lives on the size-m domain.  With M = 2 mu, rho = m / mu,
 * W = fr_root_of_unity(log2 M) and psi = omega^l:
 *   s^(e) = (P^(e)_(mu-2), .., P^(e)_0, infinity x (mu + 1))
 *   t^(e) = (c^(e)_(mu-1), 0 x (mu + 1), c^(e)_1, .., c^(e)_(mu-2))          (mu = 2: (c^(e)_1, 0, 0, 0))
 *   h = the first mu entries of IDFT_M( sum_e DFT_M(s^(e)) o DFT_M(t^(e)) )
 *   (pi_0 .. pi_(m-1)) = DFT_m, root psi, of (h_0 .. h_(mu-2), infinity x (m - mu + 1))
 * bbgpu_kzg_open_cosets_setup_bounded makes a setup of this kind in the pool of the block above (BBGPU_KZG_OPEN_COSETS_MAX_SETUPS setups in all, bounded or
 * not); the handle is used with bbgpu_kzg_open_cosets_device and bbgpu_kzg_open_cosets_release -- there is no second device entry.
 *   degree_bound a power of two with 2 x coset <= degree_bound <= n, otherwise BBGPU_ERR_SIZE, refused before a device is bound as the sizes of the block
 *                above are.  degree_bound == n IS bbgpu_kzg_open_cosets_setup(srs_handle, n, coset): the same rows read, the same footprint, the same
 *                launches and proofs (that entry is this call).
 *   the table    rows [0, d - l) are read and curve-checked (a bad row: BBGPU_ERR_ARG naming the first one, no setup is made); rows from d - l on are not
 *                read, and the table need hold no more than d rows: a string of d rows opens on the domain of size n = d, 2 d, 4 d, .. up to 2^21.  A table of
 *                fewer than d rows: BBGPU_ERR_SIZE.
 *   footprint    l x M = 2 d rows of S^ (2 d x 128 bytes, counted in bbgpu_memory_info.staging_bytes while the setup lives).
 * Over a bounded setup bbgpu_kzg_open_cosets_device reads coefficients [0, d) of each polynomial and NOTHING FROM d ON: WHAT LIES AT [d, stride_elems) IS
 * NOT READ AND NOT CHECKED -- a polynomial whose coefficients there are not zero gets the proofs of its truncation to degree < d, which hold for no
 * commitment of the whole polynomial.  stride_elems >= d is accepted (BBGPU_ERR_SIZE below d), so the d_coeffs_out of bbgpu_kzg_recover_cells goes in with
 * that call's stride.  The batch rule stays that of the domain: batch in 1..64, batch x 2 n <= 2^22.  The result is the same batch x m proofs in the same
 * format and natural order; for a polynomial whose coefficients from d on are zero they are the proofs of an unbounded setup bit for bit (unique affine
 * points).  coset == 1 through this entry is the bounded form of bbgpu_kzg_open_all_device, which has no bound of its own.
 * The kernels (csrc/kzg_open_cosets.hip) tell mu from m: k_open_cosets_string, k_open_cosets_t and k_open_cosets_sum run at size M = 2 mu -- l x M = 2 d
 * threads and ladders, source rows and coefficients below d; the inverse transform is log2 M launches of k_lagrange_stage over M slots;
 * k_open_cosets_gather REPLICATES: slot m + rho bitrev_mu(u) + c <- h_u for u < mu - 1 and every c < rho, the rho slots of u = mu - 1 <- infinity.  The
 * stage kernel is a decimation in time over bit-reversed input, whose nonzero entries sit at multiples of rho here, so its first log2 rho stages would
 * only turn (a, infinity) into (a, a); the gather writes those copies and only stages log2 rho .. log2 m - 1 are launched.  k_open_cosets_finish is
 * unchanged.  Every polynomial keeps 2 m scratch slots whatever d is (the convolution in [0, M), the forward transform in [m, 2 m)), and the buffer of
 * the scalars, which later holds the proofs, has the larger of batch x 2 d x 32 and batch x m x 64 bytes (the proofs outgrow the scalars when d < m, as
 * at (1024, 1, 4)).  The gather: 38 VGPRs (16 SGPRs), no LDS, no scratch memory, 8 waves per SIMD -- the figures of the gather it replaces; the other kernels
 * as in the block above; no scratch memory in any kernel (the compiler's resource remarks, at the head of profiles/kzg_open_bounded.txt).
 * A warm setup and a warm call at (n, l, d) = (512, 4, 256) pass the funnels of the block above at (256, 4): setup -- one allocation, one upload, one
 * read-back, two launch checks; call -- two allocations, no upload, one read-back, three launch checks.  After a failure nothing the call allocated is
 * live and the setup stays usable.  bbgpu_set_timing(1) reports the same four device times with the same meaning.
 * Cost on one MI355X (tools/kzg_open_bounded_bench.py, profiles/kzg_open_bounded.txt): wall ms per call at d = n / 2, l = 64, proofs read back to the host, one
 * box, against THE SAME ENTRY over a setup without a bound fed the same coefficients zero-padded, timed in the same process in alternating pairs (medians
 * of 9 pairs, 3 at 2^20).  n = 2^12: 12.8 ms against 13.0 (batch 16: 15.3 against 16.2); n = 2^16: 19.9 against 22.0 (batch 16: 35.9 against 51.6);
 * n = 2^20: 43.6 against 59.4.  By the rule of the block above -- a leg wins a shape when its median is lower by more than the full range (max - min) of
 * either leg -- the bounded setup wins four of the five shapes, (2^16, 64) and (2^20, 64) among them, and loses none: at (2^12, 64), batch 1, its median is
 * lower by 0.25 ms, WITHIN the spread of 0.48 -- a call of one small polynomial is bound by the latency of its stage launches, of which the bound saves two
 * of 13, one of them the forward stage 0, which runs no ladder.  Device times at (2^20, 64), bounded against unbounded: the sum kernel 16.7 ms against 31.2, the inverse stages 13.1 against 14.0, the gather and
 * the forward stages 13.1 against 13.1, the finish kernel 0.16 against 0.16 -- the ladders halve, one inverse stage fewer at half the length saves 1 ms, and
 * the forward transform does not move: the stage it loses was a launch over copies.  The setup, with its release: 88.3 ms against 186.6 at 2^20, 9.6
 * against 10.8 at 2^16, 7.0 against 6.5 at 2^12 (not paired; at that size the setup is bound by its launches).  NOT timed: other ratios d / n, l < 64, the
 * host twin.  Nothing was tuned after these measurements.
 * The host twin (csrc/host_kzg_open_cosets.hpp) restates the construction with the twin's own transforms and runs ALL log2 m stages of the last transform
 * over the zero-padded input -- not the replicating gather -- so that device and twin check each other; bbgpu_host_kzg_open_cosets is its d = n case.  It
 * reads rows [0, d - l) of the table and coefficients [0, d); its errors are those of the device entries. */
int bbgpu_kzg_open_cosets_setup_bounded(int srs_handle, size_t n, size_t coset, size_t degree_bound); /* setup handle >= 0, of the pool above */
int bbgpu_host_kzg_open_cosets_bounded(const uint64_t* points_endo_table, size_t n, size_t coset, size_t degree_bound, const uint64_t* coeffs,
                                       size_t stride_elems, int batch, uint64_t* proofs_out /* batch x (n / coset) x 8 */);

/* ---- do these openings hold?  (up to 2^20 KZG claims: the per-claim rows and scalars on the GPU, one pairing check) ------
 * bbgpu_host_kzg_check_openings above is host only and takes 64 claims; one call of bbgpu_kzg_open_all_device writes up to 2^20 proofs, and a
 * data-availability verifier receives thousands of (commitment, point, value, proof) claims per request.  These entries check `count` claims -- "the
 * polynomial behind the claim's commitment takes the value y_t at z_t, with proof point pi_t" -- in one call, by the same definition:
 *   A = sum_t rho_t C_t + sum_t (rho_t z_t) pi_t - (sum_t rho_t y_t) G,   B = sum_t rho_t pi_t,   ok = ( e(A, G2) e(-B, x G2) == 1 )
 * rho_t = bbgpu_srs_check's multipliers Keccak-256(seed || t) with the top three bits cleared, t the claim's position in the caller's arrays, handed to
 * the sums as they are; the seed rules are the same (NULL: 32 bytes from the operating system; THE SEED MUST NOT BE KNOWN TO WHOEVER MADE THE PROOFS; it
 * is reported afterwards so that a finding can be replayed).  The soundness error is about 2^-253 per check.  All pointers are HOST memory; points are
 * affine {x, y} in the reference's format, the infinity flag honoured; z / y: 4 words each, any representative below 2^256.
 * bbgpu_kzg_check_openings has two layouts:
 *   which == NULL   commitments holds count x 8 words, one per claim: exactly bbgpu_host_kzg_check_openings; num_commitments is not read.
 *   which != NULL   1 <= num_commitments <= BBGPU_KZG_CHECK_MAX_COMMITMENTS shared commitments, claim t is of commitments[which[t]] (the labelling of
 *                   bbgpu_plonk_verify_multi); the sum over the commitments becomes sum_c (sum_{t: which[t] = c} rho_t) C_c.
 * bbgpu_kzg_check_open_all is the shared layout for what bbgpu_kzg_open_all_device writes: claim t = b n + i has commitment b, z_t = omega^i (made on
 * the device, omega the root of the size-n domain), y_t = values[(b * stride + i) * 4] and pi_t = proofs[(b * n + i) * 8].
 * Return codes: BBGPU_OK means the check RAN; the verdict is report.ok.  Refused before a device is bound -- BBGPU_ERR_SIZE: count outside 1 ..
 * BBGPU_KZG_CHECK_MAX_CLAIMS, n not a power of two, batch outside 1..64, stride < n, batch x n > 2^20; BBGPU_ERR_ARG: a null pointer, num_commitments outside
 * 1..64, a which[t] >= num_commitments, unknown flag bits, a g2_x that bbgpu_srs_check would not take.  Unlike bbgpu_host_kzg_check_openings, a finite point
 * off the curve is a FINDING, not an argument error: bad_points counts them among commitments and proofs, first_bad names the first (a shared commitment
 * by its own index before any claim; in the per-claim layout C_t before pi_t), ok = 0, rounds = 0 and no MSM is issued.  Points at infinity are legal and add
 * nothing (the proof of a constant polynomial is infinity).
 * The kernels (csrc/kzg_check.hip): k_kzg_claims takes one claim per thread, strided -- rho_t by csrc/keccak_device.hpp, pi_t (and C_t in the per-claim
 * layout) by 16-byte loads, the curve test of k_srs_on_curve, the point as a resident row (the generator under scalar zero for infinity), the scalars rho_t
 * for B and rho_t z_t for A by one product with rho_t read as an integer (the twin's fr_mul), the term rho_t y_t; in the open-all form z_t starts from
 * square-and-multiply on i and advances by one product per stride.  Findings meet in the wave and in one LDS slot per wave; one thread per workgroup issues
 * the atomics, an honest call none.  k_kzg_fold (at most 256 ranges of claims, then k_kzg_fold_finish when there is more than one range) writes -sum rho_t y_t
 * on G and sum_{which[t] = c} rho_t on C_c for the first m claims: canonical additions modulo r in a fixed tree, no atomics, no floating point.  A and B are
 * the existing device MSM over the rows as transient tables -- ONE table, read by A from its head and by B from the first claim on -- and the pairing
 * is one bbgpu_host_pairing_check of two pairs.  BBGPU_KZG_CHECK_LOCATE: after a failed check the prefix length is bisected (at most ceil(log2 count) more
 * rounds of fold, two MSMs and pairing, no new buffer): first_failing is the smallest t such that claims [0, t] fail.
 * The entries run on context 0 under the library mutex.  One staging buffer (the caller's arrays, the rows, both scalar arrays, the terms, the partial
 * sums, the findings: 288 bytes per claim in the open-all form, 324 in the shared layout with labels, 480 in the per-claim layout, i.e. 503 MB at 2^20
 * claims) is kept between calls, counted in bbgpu_memory_info.staging_bytes and released by bbgpu_shutdown.  Uploads go through the library's
 * host_to_device (pinned staging in 1 MiB chunks up to 8 MiB, the direct copy above); the shared rows are converted on the host and sent with the
 * findings' start value in one copy.  A warm call of 256 claims passes no allocation, one read-back (the findings), four launch checks (k_kzg_claims,
 * k_kzg_fold, one per MSM ticket) and five uploads in the per-claim layout (proofs, y, z, commitments, the head) and with labels (labels in place of the
 * commitments), three in the open-all form (proofs, values, the head; one more per polynomial when stride > n); with a finding one launch check.
 * After any failure no MSM ticket is outstanding.  With the same seed the report equals the host twin's field for field, a and b included.
 * The host twins (csrc/host_kzg_check_batch.hpp) are plain loops over the host bucket method and the host pairing: no HIP call, no lock.
 * Cost on one MI355X (tools/kzg_check_bench.py, profiles/kzg_check.txt; wall ms per call, one box, the claims of ONE polynomial): open-all form 1.69 ms at
 * 256 claims, 1.90 at 4096, 2.66 at 2^16, 7.08 at 2^20; per-claim layout 1.82 / 2.00 / 3.51 / 10.95.  Up to 2^16 claims a call is the two MSMs plus the
 * 1.0 ms host tail (the pairing check); at 2^20 the open-all form spends 2.3 ms on the uploads (96 MB) and k_kzg_claims, 3.5 ms in the MSMs, 1.0 ms in
 * the tail -- the upload does not dominate.  The path there was before, bbgpu_host_kzg_check_openings over 64 claims at a time: 2.4-2.6 ms per call,
 * timed on 8 chunks and SCALED (an extrapolation) 9.9 ms, 156 ms, 2.6 s and 41 s.  NOT measured: the kernels alone from events, the labelled layout at
 * the large sizes, the rounds of LOCATE, several polynomials per call.  Nothing was tuned. */
#define BBGPU_KZG_CHECK_MAX_CLAIMS      (1u << 20)
#define BBGPU_KZG_CHECK_MAX_COMMITMENTS 64
#define BBGPU_KZG_CHECK_LOCATE          1
typedef struct {
    uint64_t count;              /* claims in the call */
    uint64_t bad_points;         /* finite points off the curve among commitments and proofs */
    uint64_t first_bad;          /* claim index (commitment index if it is a shared commitment), UINT64_MAX if none */
    uint32_t first_bad_is_proof; /* the first finding is claim first_bad's proof, not a commitment */
    uint32_t g2_ok;              /* 1: a g2_x that is not usable is refused with the arguments */
    uint32_t ok;                 /* bad_points == 0 and e(A, G2) e(-B, x G2) == 1 */
    uint32_t rounds;             /* rounds of fold, two MSMs and pairing: 0 with findings, 1, or 1 + the bisection's */
    int64_t first_failing;       /* with BBGPU_KZG_CHECK_LOCATE after a failed check: smallest t such that claims [0, t] fail; -1 otherwise */
    uint64_t seed[4];            /* the seed in use */
    uint64_t a[8], b[8];         /* A and B, affine (infinity flag honoured; infinity when no sums were taken) */
} bbgpu_kzg_check_report;
int bbgpu_kzg_check_openings(const uint64_t* commitments, const uint32_t* which /* NULL: one commitment per claim */, size_t num_commitments,
                             const uint64_t* z /* count x 4 */, const uint64_t* y /* count x 4 */, const uint64_t* proofs /* count x 8 */, size_t count,
                             const uint64_t g2_x[16], const uint64_t seed[4] /* NULL: OS randomness */, int flags, bbgpu_kzg_check_report* report);
int bbgpu_kzg_check_open_all(const uint64_t* commitments /* batch x 8 */, const uint64_t* values /* batch x stride x 4 */, size_t stride,
                             const uint64_t* proofs /* batch x n x 8 */, size_t n, int batch, const uint64_t g2_x[16], const uint64_t seed[4], int flags,
                             bbgpu_kzg_check_report* report);
int bbgpu_host_kzg_check_openings_batch(const uint64_t* commitments, const uint32_t* which, size_t num_commitments, const uint64_t* z, const uint64_t* y,
                                        const uint64_t* proofs, size_t count, const uint64_t g2_x[16], const uint64_t seed[4], int flags,
                                        bbgpu_kzg_check_report* report);
int bbgpu_host_kzg_check_open_all(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, int batch,
                                  const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report);
/* wall ms of the last bbgpu_kzg_check_* call between the synchronisations it makes anyway: total, uploads and k_kzg_claims, folds, MSMs, host tail */
int bbgpu_kzg_check_last_timing(double ms_out[5]);

/* ---- do these CELL proofs hold?  (a batch of cells of bbgpu_kzg_open_cosets_device: the interpolation polynomials on the GPU, one pairing check) ------
 * bbgpu_kzg_open_cosets_device writes the n / l cell proofs a data-availability sampler ships; the entries above take single-point claims only.  These
 * check `count` cells.  Notation: l = coset, m = n / l, omega = fr_root_of_unity(log2 n), psi = omega^l, zeta = omega^m.  Cell k < m of the polynomial f
 * holds v_j = f(omega^(k + m j)), j < l in natural order -- the entries k, k + m, k + 2 m, .. of the caller's size-n bbgpu_ntt_device, as the open-cosets
 * block says -- and its proof pi_k has f = q_k (X^l - psi^k) + r_k, where r_k = sum_i a_{k,i} X^i is the interpolation polynomial of the cell:
 *   a_{k,i} = omega^(-k i) l^-1 sum_j v_j zeta^(-i j)                    (a size-l inverse transform, then a twist)
 * For cells t < count, each (commitment label c_t, cell index k_t, l values, pi_t), rho_t the multipliers of bbgpu_srs_check by the cell's position:
 *   s_i = sum_t rho_t a_{t,i}                                                                   (i < l)
 *   A   = sum_c (sum_{t: c_t = c} rho_t) C_c - sum_{i < l} s_i P_i + sum_t (rho_t psi^(k_t)) pi_t,     B = sum_t rho_t pi_t
 *   ok  = ( e(A, G2) e(-B, [x^l] G2) == 1 )
 * g1_head holds P_0 .. P_(l-1), the first l rows of the monomial string (affine, the reference's format).  g2_xl = [x^l] G2 IS A VERIFIER-KEY ITEM THE
 * CALLER SUPPLIES: a transcript that carries only x G2 CANNOT verify cells for l > 1 (x^l G2 does not follow from x G2 without the secret).
 * bbgpu_host_kzg_cells_key_check says whether a g2_xl belongs to a head and an x G2: g2_xl on the twist, finite, of order r, and
 * e(P_(l-1), g2_x) e(-G, g2_xl) == 1 -- one bbgpu_host_pairing_check of two pairs; host only, no lock, re-entrant; at l = 1 it says whether g2_xl == g2_x as
 * points.  A head row, g2_x or g2_xl it cannot use gives *ok = 0; BBGPU_ERR_SIZE: coset not a power of two in 1..64, BBGPU_ERR_ARG: a null pointer.
 * At l = 1 with P_0 = G and g2_xl = g2_x, A and B are exactly those of bbgpu_kzg_check_open_all, and so is the report.
 * bbgpu_kzg_check_cells is the labelled form: cell t is cell cell[t] of commitments[which[t]], its l values at values[(t l + j) * 4]; the same (label,
 * cell) twice is legal.  bbgpu_kzg_check_open_cosets is exactly what bbgpu_kzg_open_cosets_device writes: cell t = b m + k has label b and cell k, pi_t =
 * proofs[(b m + k) * 8], and its values are gathered ON THE DEVICE from the transform at values[b * stride * 4], m elements apart (no host transpose).
 * The report is bbgpu_kzg_check_report with `count` in cells; flags, seed rules, the soundness error and the meaning of BBGPU_OK are those of
 * bbgpu_kzg_check_openings.  Values: any representative below 2^256.  Points at infinity are legal: a polynomial of degree below l has every proof at
 * infinity, A and B are then both infinity and ok = 1; a commitment at infinity is the zero polynomial.
 * Refused before a device is bound -- BBGPU_ERR_SIZE: coset not a power of two in 1 .. BBGPU_KZG_OPEN_COSETS_MAX_COSET, n not a power of two, n / coset < 2,
 * n > 2^21, count outside 1 .. 2^20, count x coset > 2^20, batch outside 1..64, stride < n (batch x n > 2^20 is count x coset > 2^20); BBGPU_ERR_ARG: a null
 * pointer, num_commitments outside 1..64, a which[t] >= num_commitments or a cell[t] >= n / coset, unknown flag bits, a g2_xl that bbgpu_srs_check would not
 * take, a g1_head row at infinity or off the curve (it is a key, not a claim; bbgpu_last_error() names the first such row).  A commitment or a proof that
 * is finite and off the curve is a FINDING as in the entries above: bad_points, first_bad (a commitment by its own index before any cell),
 * first_bad_is_proof, ok = 0, rounds = 0, no MSM.  BBGPU_KZG_CHECK_LOCATE: first_failing is the smallest t such that cells [0, t] fail.
 * The kernels (csrc/kzg_check_cells.hip).  k_kzg_cells takes one cell per thread, strided, as k_kzg_claims takes a claim: rho_t (kept in memory for the
 * two kernels below), the curve test of pi_t and its resident row, rho_t psi^(k_t) for A (psi^k by square-and-multiply over log2 m bits) and rho_t for B;
 * findings meet on chip, an honest call issues no atomic.  k_kzg_cell_coefficients gives a cell to l NEIGHBOURING LANES -- a wave takes 64 / l cells, a
 * workgroup 256 / l, strided over at most 1024 workgroups; lanes of a cell past the end compute on zeros, so every lane reaches every barrier and
 * exchange.  Each lane loads one value by two 16-byte loads (open-cosets form: the workgroup loads transposed, neighbouring threads neighbouring cells,
 * 256 / l x 32 bytes in a row, and hands the words over through 8 KiB of LDS), brings it into the field and divides by l in one product, runs the log2 l
 * decimation-in-frequency stages across lanes -- the partner's nine limbs by __shfl_xor, ONE product per lane and stage, roots from a table of l <= 64
 * entries that arrives with the head --, applies the twist omega^(-k i) (square-and-multiply over the log2 n bits of k i mod n) and rho_t read as an
 * integer, and writes the canonical term T_{t,i} = rho_t a_{t,i}, which the fold and LOCATE read again: 2 log2 n + log2 l + 3 field products per value, 60
 * (labelled) / 65 (open-cosets) VGPRs, no scratch.  k_kzg_cells_fold (at most 256 ranges of cells x (S + l) slots, then k_kzg_cells_fold_finish when there is
 * more than one range) writes sum_{c_t = c} rho_t on C_c and r - s_i on P_i (zero stays zero) for the first m cells: canonical additions in a fixed tree, no
 * atomics, no floating point.  The rows are ONE transient table -- the S commitments, P_0 .. P_(l-1), then pi_t -- read by A from its head and by B from
 * the first cell on, so a prefix of the cells is a prefix of both sums.  All values are exact residues written canonically: with the same seed the
 * report equals the host twin's field for field, a and b included.
 * The entries run on context 0 under the library mutex and use the staging buffer of the entries above (224 + 64 l bytes per cell, 8 more with labels:
 * 71 MB at 2^20 values in cells of 64), kept between calls and counted in staging_bytes.  The head -- the roots, the findings' start value, the shared rows,
 * P_0 .. P_(l-1) -- is converted on the host and sent in one copy.  A warm call of 256 cells at l = 4 passes no allocation, one read-back (the findings),
 * five launch checks (k_kzg_cells, k_kzg_cell_coefficients, k_kzg_cells_fold, one per MSM ticket) and five uploads in the labelled form (proofs, values,
 * labels, cell indices, the head), three in the open-cosets form (proofs, values, the head; one more per polynomial when stride > n); with a finding two
 * launch checks (no fold, no ticket).  After any failure no MSM ticket is outstanding.  bbgpu_kzg_check_last_timing reports these entries too: index 1 is
 * the uploads and the two cell kernels.  With bbgpu_set_timing, bbgpu_last_timing gives the coefficient kernel alone (index 0, device events).
 * The host twins (csrc/host_kzg_check_cells.hpp) are plain loops -- a size-l transform per cell over host_fr.hpp, the host bucket method, the host
 * pairing: no HIP call, no lock.
 * Cost on one MI355X (tools/kzg_check_cells_bench.py, profiles/kzg_check_cells.txt; wall ms per call, one box, open-cosets form, medians of 9):
 * (n, l, batch) = (2^12, 64, 1) 1.74, (2^16, 64, 1) 1.95, (2^16, 64, 16) 3.02, (2^16, 4, 1) 2.20, (2^20, 64, 1) 3.09.  At 2^20 values the uploads (32 MB) and
 * the two cell kernels are 1.05-1.10 ms, the fold 0.03, the two MSMs over 16384 rows 0.69, the host tail (the pairing) 1.01.  k_kzg_cell_coefficients alone
 * from events: 0.297 ms at (2^16, 64, 16) and 0.352 ms at (2^20, 64, 1), beside 0.287 and 0.343 ms for the product count at the 150 Gmul/s of
 * fe_mont_gfx950.h.  Against bbgpu_kzg_check_open_all over the SAME 2^20 values at (n, batch) = (2^16, 16), alternating pairs in one process: 3.07 ms
 * against 7.15, beyond the full range of either leg (0.14).  NOT measured: the rounds of LOCATE, the labelled form at large sizes.  Nothing was tuned. */
int bbgpu_kzg_check_cells(const uint64_t* commitments /* num_commitments x 8 */, size_t num_commitments, const uint32_t* which /* count */,
                          const uint32_t* cell /* count, each < n / coset */, const uint64_t* values /* count x coset x 4 */,
                          const uint64_t* proofs /* count x 8 */, size_t count, size_t n, size_t coset, const uint64_t* g1_head /* coset x 8 */,
                          const uint64_t g2_xl[16], const uint64_t seed[4] /* NULL: OS randomness */, int flags, bbgpu_kzg_check_report* report);
int bbgpu_kzg_check_open_cosets(const uint64_t* commitments /* batch x 8 */, const uint64_t* values /* batch x stride x 4: the size-n transforms */,
                                size_t stride, const uint64_t* proofs /* batch x (n / coset) x 8 */, size_t n, size_t coset, int batch,
                                const uint64_t* g1_head /* coset x 8 */, const uint64_t g2_xl[16], const uint64_t seed[4], int flags,
                                bbgpu_kzg_check_report* report);
int bbgpu_host_kzg_check_cells(const uint64_t* commitments, size_t num_commitments, const uint32_t* which, const uint32_t* cell, const uint64_t* values,
                               const uint64_t* proofs, size_t count, size_t n, size_t coset, const uint64_t* g1_head, const uint64_t g2_xl[16],
                               const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report);
int bbgpu_host_kzg_check_open_cosets(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, size_t coset,
                                     int batch, const uint64_t* g1_head, const uint64_t g2_xl[16], const uint64_t seed[4], int flags,
                                     bbgpu_kzg_check_report* report);
/* *ok = 1 when g2_xl is [x^coset] G2 for the x of g1_head and g2_x; host only, no lock, re-entrant */
int bbgpu_host_kzg_cells_key_check(const uint64_t* g1_head /* coset x 8 */, size_t coset, const uint64_t g2_x[16], const uint64_t g2_xl[16], int* ok);

/* ---- do the cell proofs of a 2-D LAYOUT hold?  (up to 2^16 commitments in one call, still one pairing check) ------
 * bbgpu_g1_ntt, bbgpu_g1_recover and bbgpu_g1_recover_each give the commitments of the extension rows in columns of up to 2^16 points; the two entries
 * above take 64 commitments, so a layout of 256 data rows and 256 extension rows was at least eight calls, the cells partitioned by label on the host,
 * each call with its own two MSMs and its own pairing.  These entries are the SAME definition -- rho_t, A, B, the pairing product, the findings,
 * BBGPU_KZG_CHECK_LOCATE, the seed rules, the report: everything the block above says -- with two differences:
 *   num_commitments, and batch in the open-cosets form, may be 1 .. BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS = 2^16 (the tallest column the group entries
 *   write); every other bound stays: count <= 2^20, count x coset <= 2^20, n <= 2^21, n / coset >= 2, coset a power of two <= 64, stride >= n,
 *   batch x n <= 2^20.
 * Refusals come before a device is bound with the codes of the block above (BBGPU_ERR_SIZE for batch, BBGPU_ERR_ARG for num_commitments or a label >=
 * num_commitments).  The entries above, their limit of 64 and their refusals are unchanged.  For num_commitments <= 64 and the same seed the report
 * equals that of the entry above field for field, a and b included: every sum is an exact canonical residue, whatever order it is added in.
 * The device path (csrc/kzg_check_cells.hip; the driver is kzg_cells_run in capi.hip with its `layout` argument, which shares k_kzg_cells,
 * k_kzg_cell_coefficients, the tail, the two tickets over one transient table and the staging buffer with the entries above):
 *   k_kzg_layout_commitments  the commitments go up AS THEY ARE, one more upload, and are tested and converted on the device: one thread per commitment,
 *                             the device function k_kzg_cells applies to a proof (the curve test, the resident row).  A finite point off the curve is a
 *                             finding keyed by its own index; a wave writes the infinity flags of its 64 commitments as one word of a skip array.  The
 *                             findings come down with the cells' in the one read-back; the host runs no loop over the commitments (the O(count) label
 *                             validation stays).
 *   the grouping              labelled form, once per call: k_kzg_layout_hist (integer atomics on S counters, one per wave and label), k_kzg_layout_scan (one workgroup: the starts
 *                             of the S lists and of their pieces), k_kzg_layout_scatter (a permutation of the cells, label by label).  O(count + S).
 *   the grouped fold          per round: k_kzg_layout_pieces gives ONE WAVE a piece of at most 1024 cells of one list -- 16 canonical additions per lane
 *                             and six shuffle steps whatever the labels are, the chain k_kzg_cells_fold runs over a range of 4096 cells; a prefix m for
 *                             LOCATE is the test t < m while summing --, k_kzg_layout_finish gives one wave a label and sums its pieces, writing zero for
 *                             a commitment at infinity.  In the open-cosets form label c is the cells [c m, (c + 1) m): no grouping, the same two kernels.
 *                             O(count + S) loads and memory; no per-commitment-per-range partial buffer.
 *   the l slots of P_i        k_kzg_cells_fold as above, called with no commitment slot.  The table of A is P_0 .. P_(l-1), the S commitments, then pi_t:
 *                             the head -- roots, the findings' start, P_0 .. P_(l-1) -- still arrives in one copy.
 * No scratch in any of them; VGPR counts in the file's header block.  Staging beyond the entries above: 76 bytes per commitment and 4 per cell in the
 * labelled form, 64 per commitment and 32 per 1024 cells in the open-cosets form, and 32 bytes per piece; counted in staging_bytes.  A warm call of 256
 * cells at l = 4 passes no allocation, ONE read-back, seven launch checks (k_kzg_cells, k_kzg_cell_coefficients, the commitments with the grouping,
 * k_kzg_cells_fold, the grouped fold, one per MSM ticket) and six uploads in the labelled form (proofs, values, labels, cell indices, commitments, the
 * head), four in the open-cosets form; with a finding three launch checks.  After any failure no MSM ticket is outstanding.  With bbgpu_set_timing,
 * bbgpu_last_timing gives device times from events: index 0 the coefficient kernel, 1 the commitments and the grouping, 2 the grouped fold of the
 * first round.
 * The host twins are the plain loops of csrc/host_kzg_check_cells.hpp with the cap as a parameter: one text for both families.
 * Cost on one MI355X (tools/kzg_check_layout_bench.py, profiles/kzg_check_layout.txt; wall ms per call, medians of 9 in alternating pairs in one process,
 * with the spread -- the full range -- of each leg; the box is shared and two legs of the run hold one outlier each, which the spread shows):
 *   (rows, n, l) = (512, 2^11, 64), 2^20 values, open-cosets form: ONE layout call 3.01 ms (spread 0.07) against 16.26 ms for the eight calls of 64 rows
 *   (fastest 16.15): 0.19 of the time.
 *   (64, 2^14, 64) against the one bbgpu_kzg_check_open_cosets call it replaces: 3.008 ms (spread 0.135) against 2.994 (fastest 2.976, one call of 6.7 ms):
 *   +0.014 ms, no slower beyond the spread of either leg (the run before, without outliers: +0.013 ms with spreads 0.063 and 0.031).
 *   the labelled form, 2^14 cells of 64 values under 512 labels: uniform labels 3.073 ms, every cell on ONE label 3.088 (spread 0.066; the uniform leg
 *   holds one call of 4.5 ms, its other calls lie within 0.05): +0.015 ms, within the spread.  From device events: the commitments kernel with the grouping
 *   0.027 ms uniform and 0.021 ms on one label, the grouped fold 0.013 and 0.024 ms.
 * The grouping was changed ONCE after a measurement: with one atomic per cell the one-label call took 3.451 ms against 3.072 (+0.379 ms, NOT within the
 * spreads of 0.05-0.07), the grouping 0.387 ms against 0.017 -- 2^14 atomics on one counter in the histogram and again in the scatter.  The lanes of a wave
 * that hold the same label now meet first (ballots, at most 64 trips, no memory access) and their leader issues one atomic: a counter takes one atomic per
 * wave that holds its label.  That costs the uniform call 0.010 ms.  At l = 1 a call of 2^20 cells on one label still puts 2^14 atomics on one counter.
 * NOT timed: the rounds of LOCATE, num_commitments above 512, the labelled form above 2^14 cells, l < 64, the host twins. */
#define BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS (1u << 16)
int bbgpu_kzg_check_cells_layout(const uint64_t* commitments /* num_commitments x 8 */, size_t num_commitments, const uint32_t* which /* count */,
                                 const uint32_t* cell /* count, each < n / coset */, const uint64_t* values /* count x coset x 4 */,
                                 const uint64_t* proofs /* count x 8 */, size_t count, size_t n, size_t coset, const uint64_t* g1_head /* coset x 8 */,
                                 const uint64_t g2_xl[16], const uint64_t seed[4] /* NULL: OS randomness */, int flags, bbgpu_kzg_check_report* report);
int bbgpu_kzg_check_open_cosets_layout(const uint64_t* commitments /* batch x 8 */, const uint64_t* values /* batch x stride x 4: the size-n transforms */,
                                       size_t stride, const uint64_t* proofs /* batch x (n / coset) x 8 */, size_t n, size_t coset, int batch,
                                       const uint64_t* g1_head /* coset x 8 */, const uint64_t g2_xl[16], const uint64_t seed[4], int flags,
                                       bbgpu_kzg_check_report* report);
int bbgpu_host_kzg_check_cells_layout(const uint64_t* commitments, size_t num_commitments, const uint32_t* which, const uint32_t* cell,
                                      const uint64_t* values, const uint64_t* proofs, size_t count, size_t n, size_t coset, const uint64_t* g1_head,
                                      const uint64_t g2_xl[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report);
int bbgpu_host_kzg_check_open_cosets_layout(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n,
                                            size_t coset, int batch, const uint64_t* g1_head, const uint64_t g2_xl[16], const uint64_t seed[4], int flags,
                                            bbgpu_kzg_check_report* report);

/* ---- recover polynomials from a subset of their cells  (the vanishing polynomial of the missing cells on the GPU, three transforms, a verdict) ------
 * bbgpu_kzg_open_cosets_device makes the n / l cell proofs of a polynomial and bbgpu_kzg_check_cells / bbgpu_kzg_check_open_cosets check them.  A node that
 * samples cells holds SOME cells of each polynomial, usually the same columns of many rows, and must rebuild the polynomials: the missing cells, and then
 * their proofs through the producer.  bbgpu_kzg_recover_cells does the first on the device and leaves the coefficients where the producer reads them.  The
 * reference has no counterpart.  Notation as in the two blocks above: l = coset, m = n / l, omega = the n-th root of the transforms, psi = omega^l, g the
 * coset generator of BBGPU_COSET_FFT; cell k < m holds f(omega^(k + m j)), j < l, and vanishes under X^l - psi^k.
 * Given the degree bound d (deg f < d <= n) and `count` distinct cells with count * l >= d, the same for all `batch` polynomials -- the column-custody case,
 * which makes the vanishing polynomial a once-per-call cost; different sets are one call each, or ONE call of bbgpu_kzg_recover_cells_each below -- let K be the mu = m - count missing cells and
 *   Z(X) = prod_{k in K} (X^l - psi^k),   z_a = prod_{k in K} (psi^a - psi^k) = Z(omega^i),   z'_a = prod_{k in K} (g^l psi^a - psi^k) = Z(g omega^i),   a = i mod m.
 * z_a is zero exactly on the missing cells, z'_a never (g^n != 1), and Z never exists in coefficient form.  Per polynomial:
 *   E_i = v_i z_(i mod m) on the present cells, 0 on the missing ones      the values of f Z on the whole domain, deg f Z < n
 *   P = IFFT(E);   Q = COSET_FFT(P);   Q_i *= 1 / z'_(i mod m);   D = COSET_IFFT(Q) = f                one batch inversion of m values per call
 * D always has degree < count * l.  The cells are values of ONE polynomial of degree < d if and only if coefficients [d, count * l) of D are all zero: an
 * exact statement, not a probabilistic one -- one altered value among redundant cells always shows.  With count * l == d there is no redundancy: ANY values
 * are the values of a polynomial of degree < d, the report says consistent = 1 and cannot say otherwise.  An inconsistent polynomial is still written (D as
 * computed) with consistent = 0 and the return value stays BBGPU_OK: a finding, not an error, as in the check entries.
 *   values        HOST, batch x count x coset x 4 words: polynomial b, listed cell t, point j; any representative below 2^256 in the reference's memory format
 *   d_coeffs_out  DEVICE, polynomial b at element b * stride_elems: coefficients [0, n) canonical Montgomery, elements [n, stride_elems) untouched -- exactly
 *                 what bbgpu_kzg_open_cosets_device and bbgpu_ntt_device take
 *   values_out    HOST or NULL: batch x n x 4, V = FFT(D), all n values, cell k at entries k, k + m, .. as everywhere else -- what bbgpu_kzg_check_open_cosets takes
 *   hip_stream    NULL = the legacy default stream; the call returns after its last copy has finished
 * Refused before a device is bound, outputs untouched -- BBGPU_ERR_SIZE: n or coset not a power of two, coset outside 1..64, n / coset < 2, n > 2^21,
 * n / coset > BBGPU_KZG_RECOVER_MAX_CELLS = 2^16, degree_bound outside 1..n, count * coset < degree_bound (too few cells), count > n / coset, batch outside
 * 1..64, stride_elems < n, batch * n > 2^22; BBGPU_ERR_ARG: a null pointer (values_out may be NULL), a cell index >= n / coset, the same cell listed twice --
 * bbgpu_last_error() names the first offender.  BBGPU_ERR_HIP with a text of its own: a nonzero coefficient in [count * l, n), which no input can cause.
 * Scope: m <= 2^16 because the vanishing values cost mu x m pairs (at most 2^15 x 2^16); larger m -- small l at large n -- is what
 * bbgpu_kzg_recover_cells_each below takes, by a product tree.  Proofs are the caller's next call: bbgpu_kzg_open_cosets_device on d_coeffs_out
 * (over a setup of bbgpu_kzg_open_cosets_setup_bounded with the same degree_bound, where that is a power of two: half the ladders at d = n / 2).
 * The kernels (csrc/kzg_recover_cells.hip; the last three take the polynomial from blockIdx.y): k_recover_roots writes psi^k for the missing cells once;
 * k_recover_vanish, the compute-bound part, gives G = min(64, 2^18 / m) neighbouring lanes to every a, walks K in LDS tiles of 256 roots with two
 * accumulators per lane (one subtraction and one product each per pair, sharing the staged root) and multiplies the G partial products in a tree across
 * lanes by __shfl_xor; bbgpu_fr_batch_invert_device's path inverts the m values z'; k_recover_scatter writes every slot of E once (values read in a row,
 * written m elements apart; no transpose through LDS: one pass of 64 bytes per element beside three transforms); k_recover_divide; k_recover_tail
 * canonicalises and finds the smallest nonzero index in [d, count * l) and in [count * l, n) per polynomial by a min-reduction on chip -- an honest call
 * issues no atomic.  The transforms are bbgpu_ntt_device_batch's, in place in d_coeffs_out at stride_elems; values_out costs a fourth on a copy.
 * Resources (hipcc -Rpass-analysis=kernel-resource-usage): k_recover_vanish 76 VGPRs, 9216 bytes of LDS, 6 waves per SIMD; k_recover_roots 41, k_recover_scatter
 * 32, k_recover_divide 32, k_recover_tail 41 VGPRs; no scratch and no spill in any.
 * It runs on context 0 under the library mutex.  A warm call at (256, 4) with values_out passes five allocations (the cell lists; z, z' and the roots; the
 * values; the findings; the copy for the forward transform -- four without values_out), three uploads (the lists, the findings' start, the values), two
 * read-backs (the findings, the transforms -- one without) and eleven launch checks (roots + vanish; the inversion's two scans and its product; scatter; four
 * transforms; divide; tail); every site failed once through bbgpu_fault_inject returns BBGPU_ERR_HIP, leaves nothing the call allocated live, and the next
 * call is bit-exact (tests/test_gpu_kzg_recover_cells.py).  With bbgpu_set_timing(1), bbgpu_last_timing() index 0 is the device time of k_recover_roots and
 * k_recover_vanish, 1 that of scatter and IFFT, 2 that of coset FFT, divide, coset IFFT and tail, 3 that of the forward transform (only with values_out).
 * Cost on one MI355X (tools/kzg_recover_cells_bench.py, profiles/kzg_recover_cells.txt): wall ms per call with values_out read back into a buffer the caller
 * keeps, one box, medians of 9 alternating pairs beside the same four bbgpu_ntt_device_batch calls alone (no copy), every other cell missing / one cell
 * missing, degree bound n / 2: (n, l, batch) = (8192, 64, 1) 0.42 / 0.42 against 0.14; (8192, 64, 64) 1.53 / 1.50 against 0.27; (2^16, 64, 16) 1.98 / 2.28
 * against 0.40; (2^20, 64, 1) 3.99 / 2.41 against 0.47; (2^20, 64, 4) 8.18 / 7.45 against 1.67.  The difference is the copies across the link (count x l x
 * 32 bytes up, n x 32 down per polynomial), the vanishing values, the inversion with its synchronisation, scatter, divide and tail.  Device times from
 * events at (2^20, 64, 1), every other cell missing: roots + vanish 1.88 ms, scatter + IFFT 0.14, coset FFT + divide + coset IFFT + tail 0.26, FFT 0.11.
 * k_recover_vanish against its own product count, 2 mu m = 2^28 at that shape, at the 150 Gmul/s of fe_mont_gfx950.h (1.79 ms): 1.05 times at batch 1 and
 * 1.18 at batch 4 in that run, 1.20 and 1.22 in the run before it -- the kernel runs near the multiplier's rate.  With the roots of each tile computed
 * inside the kernel it took 1.88 times (3.36 ms): that is why k_recover_roots exists; nothing else was tuned.  At the small shapes the kernel takes 0.03
 * to 0.05 ms whatever mu: the powers psi^a and the launch, not the pairs.  A values_out buffer allocated afresh for every call (32 MiB or more) cost 20 to
 * 30 ms per call in the host's page handling during an earlier run: keep the buffer.  NOT measured: l < 64, m near 2^16 with many cells missing (the
 * worst case, 2^32 products), the host twin.
 * The host twin (csrc/host_kzg_recover_cells.hpp; plain loops over host_fr.hpp and the radix-2 transform of host_fallback.hpp, one inversion per z'; no HIP
 * call, no lock, re-entrant) has the same refusals and the same canonical outputs: device and twin agree bit for bit, report included.  It is held to the
 * polynomial the cells came from and, at n <= 64, to Lagrange interpolation over Python integers (tests/test_kzg_recover_cells_host.py). */
#define BBGPU_KZG_RECOVER_MAX_CELLS (1u << 16)
typedef struct {
    uint32_t consistent;      /* 1: every polynomial has coefficients [d, count * coset) all zero (vacuous when count * coset == d) */
    uint32_t first_bad_poly;  /* smallest b with a nonzero coefficient there, else 0 */
    uint64_t first_bad_coeff; /* its smallest such index, else 0 */
    uint64_t missing;         /* mu = n / coset - count */
} bbgpu_kzg_recover_report;
int bbgpu_kzg_recover_cells(const uint32_t* cell /* count, distinct, each < n / coset, any order */, size_t count,
                            const uint64_t* values /* HOST, batch x count x coset x 4: polynomial b, listed cell t, point j */, size_t n, size_t coset,
                            size_t degree_bound, int batch, uint64_t* d_coeffs_out /* DEVICE, batch x stride_elems x 4 */, size_t stride_elems,
                            uint64_t* values_out /* HOST or NULL: batch x n x 4, the size-n transforms */, bbgpu_kzg_recover_report* report, void* hip_stream);
int bbgpu_host_kzg_recover_cells(const uint32_t* cell, size_t count, const uint64_t* values, size_t n, size_t coset, size_t degree_bound, int batch,
                                 uint64_t* coeffs_out /* HOST, batch x stride_elems x 4 */, size_t stride_elems, uint64_t* values_out,
                                 bbgpu_kzg_recover_report* report);

/* ---- recover polynomials whose cell sets differ, at any n / l  (the vanishing polynomials in coefficient form from a product tree) ------
 * bbgpu_kzg_recover_cells above wants the same cells of every polynomial and at most 2^16 cells, because it computes the values of Z by mu x m pair
 * products once per call.  A node that samples at random, or repairs the rows of a 2-D layout, holds a DIFFERENT set of each polynomial, and plain
 * Reed-Solomon erasure decoding (l = 1) has m = n cells.  bbgpu_kzg_recover_cells_each takes per-polynomial cell lists and any m = n / l up to n = 2^21:
 * polynomial b lists count_b = cell_offsets[b + 1] - cell_offsets[b] distinct cells with count_b * l >= d and misses the mu_b = m - count_b cells K_b.
 * Everything the block above fixes holds here too: notation, the layout of cells, the memory format of `values` (now cell_offsets[batch] x coset x 4 words
 * in the order of `cell`), what d_coeffs_out and values_out contain, canonical Montgomery outputs, "a finding, not an error" for inconsistent cells, the
 * vacuous verdict where count_b * l == d, context 0 under the library mutex, the return after the last copy.  first_bad_out, if given, receives per
 * polynomial the smallest nonzero index in [d, count_b * l), UINT64_MAX for none; the report names the first such polynomial.  The device entry
 * writes report and first_bad_out only after its last copy has succeeded.
 * Z_b(Y) = prod_{k in K_b} (Y - psi^k), Y = X^l, in COEFFICIENT form, O(m log^2 m) products, batched over the polynomials:
 *   roots    every polynomial's list is padded with ZERO roots to a common power of two M >= max mu_b (>= 1, <= m since count_b >= 1): the padded product
 *            is Y^(M - mu_b) Z_b, so Z_b's coefficients are the padded product's read from offset M - mu_b -- exact, no division, mu_b = 0 gives Z_b = 1
 *   leaves   k_each_leaves: T = min(64, M) roots -> the T low coefficients of their monic product (the leading 1 is implied everywhere in the tree), one
 *            coefficient per lane, one wave per leaf: per root c_i <- c_i - r c_(i+1) with the neighbour's nine limbs by __shfl_down and one two-product
 *            reduction (mul_add) per lane; the roots -psi^k are computed by the same lanes into LDS first (no roots kernel)
 *   levels   (X^D + a)(X^D + b) = X^(2D) + X^D (a + b) + a b with deg a b <= 2 D - 2: the low part fits a cyclic transform of size 2 D without wrap-around.
 *            Every node keeps its D low coefficients in a slot of 2 D elements, upper half zero; per level ONE batched FFT of size 2 D over all slots of
 *            all polynomials, k_each_pair -- s (A_j + B_j) + A_j B_j with s = (-1)^j = the value of X^D, written over A_j, zero over B_j -- and ONE batched
 *            IFFT of every other slot, which leaves the parent's 2 D coefficients in the low half of its slot of 4 D: three launch groups per level and no
 *            separate add or repack kernel.  The transforms are the internal ntt_device_batch (blockIdx.y = transform; calls split at 32768 transforms;
 *            the shared scratch sized per call for sizes above 2^11).  The walk visits the domain sizes 2 T .. M and then m and n once each, in
 *            ascending order, every size used at once after it is fetched: under the table cache's least-recently-used rule (BBGPU_NTT_TABLE_BYTES) a
 *            set that is dropped is one the call no longer needs, and all sets to 2^21 together hold 0.5 GiB of the default 8 GiB
 *   values   k_each_powers + k_each_gather write Z_b's mu_b + 1 coefficients x 2^5 and x (g^l)^j 2^-5 (two small power tables) zero-padded to m; ONE batched
 *            FFT of 2 batch transforms of size m gives z_b as Montgomery-261 multipliers and z'_b x 2^-5; one batch inversion over all batch x m z'
 *   the rest as above with per-polynomial lists: k_each_scatter, IFFT, COSET_FFT, k_each_divide, COSET_IFFT, k_each_tail (windows [d, count_b l) and
 *            [count_b l, n) per polynomial), the optional FFT.  csrc/kzg_recover_cells.hip is unchanged and bbgpu_kzg_recover_cells bit-identical.
 * Refused before a device is bound, outputs untouched -- BBGPU_ERR_SIZE: n or coset not a power of two, coset outside 1..64, n / coset < 2, n > 2^21,
 * degree_bound outside 1..n, batch outside 1..64, stride_elems < n, batch * n > 2^22, for some b count_b = 0, count_b > n / coset or count_b * coset <
 * degree_bound; BBGPU_ERR_ARG: a null pointer (values_out and first_bad_out may be NULL), cell_offsets[0] != 0 or offsets that decrease, a cell index >=
 * n / coset, a cell listed twice within one polynomial -- bbgpu_last_error() names the first offender by polynomial and position.  There is NO cap on
 * n / coset.  BBGPU_ERR_HIP with a text of its own: a nonzero coefficient in [count_b * l, n), which no input can cause.  Not here: a per-polynomial
 * degree bound, cells of different sizes in one call, n > 2^21.
 * Resources (hipcc -Rpass-analysis=kernel-resource-usage, VGPRs / LDS bytes / waves per SIMD): k_each_leaves 52 / 9216 / 8, k_each_pair 45 / 0 / 8,
 * k_each_powers 42 / 0 / 8, k_each_gather 41 / 0 / 8, k_each_scatter 32 / 0 / 8, k_each_divide 32 / 0 / 8, k_each_tail 41 / 32 / 8; no scratch and no
 * spill in any.
 * A warm call with values_out passes six allocations (the lists; the tree; z, z' and the power tables; the values; the findings; the copy for the forward
 * transform -- five without values_out), three uploads (the lists, the findings' start, the values), two read-backs (the findings, the transforms -- one
 * without) and, at (256, 4) where 64 cells make one leaf and no level, thirteen launch checks (leaves; powers + gather; the Z transforms; the inversion's
 * two scans and its product; scatter; four transforms; divide; tail); every tree level adds three (at (1024, 1) with 200 cells missing: nineteen).
 * Every site failed once through bbgpu_fault_inject returns BBGPU_ERR_HIP, leaves nothing the call allocated live, and the next call is bit-exact
 * (tests/test_gpu_kzg_recover_each.py).  With bbgpu_set_timing(1), bbgpu_last_timing() index 0 is the device time of leaves, levels, gather and the Z
 * transforms, 1 that of scatter and IFFT, 2 that of coset FFT, divide, coset IFFT and tail, 3 that of the forward transform (only with values_out); the
 * batch inversion lies between 0 and 1 and is in none.
 * Cost on one MI355X (tools/kzg_recover_each_bench.py, profiles/kzg_recover_each.txt; wall ms per call with values_out read back into a buffer the caller
 * keeps, one box, medians of 9 alternating pairs).  SAME set for all polynomials, this entry / bbgpu_kzg_recover_cells, every other cell missing and
 * one cell missing: (n, l, batch) = (8192, 64, 1) 0.49 / 0.43 and 0.45 / 0.43; (2^16, 64, 16) 2.30 / 2.10 and 2.40 / 2.33; (2^20, 64, 1) 2.57 / 4.19
 * and 2.48 / 2.49; (2^20, 64, 4) 6.97 / 8.32 and 7.70 / 7.44 -- the tree wins where the pair kernel has work (0.45 ms of device time against 1.88 at
 * (2^20, 64) with half the cells missing) and loses 0.02 to 0.25 ms elsewhere to its extra launches and lists; that is the figure for moving the old
 * entry onto the tree, which this change does not do.  DIFFERENT sets, a random half missing, one call here against `batch` calls there: (2^16, 64, 16)
 * 2.36 against 11.84; (2^20, 64, 4) 7.37 against 16.96.  The shapes only this entry takes, half the cells missing: (2^20, 1, 1) 10.0 ms, device times
 * tree + Z transforms 2.72, scatter + IFFT 0.16, coset FFT + divide + coset IFFT + tail 0.29, FFT 0.12; (2^20, 4, 4) 13.5 ms, device 2.27 / 0.52 / 0.99 /
 * 0.41; the rest of the wall time is the host's lists of missing cells, the copies across the link and the inversion of batch x m values.
 * T was chosen by measurement (a build with KZG_RECOVER_EACH_LEAF = 256 in csrc/bbgpu_internal.h runs a leaf on four waves that exchange through LDS behind one barrier per
 * root; kernel trace, same box): k_each_leaves 0.448 ms at T = 64, 2.00 times its product count M T per polynomial at the 150 Gmul/s of
 * fe_mont_gfx950.h (0.224 ms for 2^25; every lane and root is a two-product reduction), 1.445 ms at T = 256, 1.61 times its count (0.895 ms for 2^27);
 * the tree with the Z transforms 2.72 ms against 3.41 at (2^20, 1, 1), 2.27 against 2.99 at (2^20, 4, 4), 0.48 against 0.62 at (2^20, 64, 4): the two
 * levels T = 256 saves cost less than its leaves add, so T = 64 ships.  NOT timed: the host twin, l = 1 at batch x n = 2^22, batches in which one
 * polynomial misses far more cells than the others (all are padded to the largest M), the inversion and the host's part of a call on their own.
 * The host twin (csrc/host_kzg_recover_each.hpp) is plain loops and deliberately NOT a tree: z_b and z'_b by direct products over K_b, once per
 * polynomial, exactly as host_kzg_recover_cells.hpp does, so that it states independently what the tree must produce.  That costs sum_b mu_b x m x 2
 * products: a checker for test sizes, not a fallback for m = 2^20.  Same refusals, same canonical outputs, report and first_bad_out included; no HIP
 * call, no lock, re-entrant.  It is held to Lagrange interpolation over Python integers at n <= 64 and to bbgpu_host_kzg_recover_cells bit for bit
 * where the sets agree (tests/test_kzg_recover_each_host.py). */
typedef struct {
    uint32_t consistent;      /* 1: every polynomial b has coefficients [d, count_b * coset) all zero (vacuous where count_b * coset == d) */
    uint32_t first_bad_poly;  /* smallest b that has not, else 0 */
    uint64_t first_bad_coeff; /* its smallest such index, else 0 */
    uint64_t max_missing;     /* max over b of n / coset - count_b */
} bbgpu_kzg_recover_each_report;
int bbgpu_kzg_recover_cells_each(const uint32_t* cell_offsets /* batch + 1, cell_offsets[0] = 0, non-decreasing */,
                                 const uint32_t* cell /* cell_offsets[batch]: polynomial b owns cell[cell_offsets[b] .. cell_offsets[b + 1]), distinct, any order */,
                                 const uint64_t* values /* HOST, cell_offsets[batch] x coset x 4, in the order of `cell` */, size_t n, size_t coset,
                                 size_t degree_bound, int batch, uint64_t* d_coeffs_out /* DEVICE, batch x stride_elems x 4 */, size_t stride_elems,
                                 uint64_t* values_out /* HOST or NULL, batch x n x 4 */,
                                 uint64_t* first_bad_out /* HOST or NULL, batch: smallest nonzero index in [d, count_b * coset) of polynomial b, UINT64_MAX if none */,
                                 bbgpu_kzg_recover_each_report* report, void* hip_stream);
int bbgpu_host_kzg_recover_cells_each(const uint32_t* cell_offsets, const uint32_t* cell, const uint64_t* values, size_t n, size_t coset, size_t degree_bound,
                                      int batch, uint64_t* coeffs_out /* HOST, batch x stride_elems x 4 */, size_t stride_elems, uint64_t* values_out,
                                      uint64_t* first_bad_out, bbgpu_kzg_recover_each_report* report);

/* ---- recover missing G1 points of a codeword  (transforms whose elements are curve points, batched over short columns; erasure decoding in the group) ------
 * The three blocks above rebuild the FIELD side of a sampled 2-D layout.  Its GROUP side: k rows (polynomials) are Reed-Solomon-extended column-wise to
 * R = 2 k rows over the size-R domain; commitment and every cell proof are linear in the polynomial, so for each column c the row commitments C_r and the
 * cell proofs pi_(r, c), r < R, are a codeword whose symbols are curve points -- the values on the size-R domain of a "polynomial" of degree < k with G1
 * coefficients.  bbgpu_g1_ntt transforms such columns and bbgpu_g1_recover decodes them from a subset of their rows, without the data: a producer gets the
 * proofs of the R - k extension rows from those of the k it made, and a sampler that holds the commitments and proofs of some rows gets the rest.  The
 * reference has no counterpart.
 * Points are affine in the reference's memory format, 8 words, exactly as bbgpu_kzg_open_cosets_device writes them: coordinates Montgomery-256 and
 * CANONICAL, infinity as bit 63 of y[3] with every other word zero.  Infinity is an ordinary input and an ordinary output, and every addition is complete:
 * equal points, opposite points and infinity on either side are not errors.
 * bbgpu_g1_ntt, `batch` columns of n points: forward out_i = sum_j rho^(i j) P_j with rho = fr_root_of_unity(log2 n), the root bbgpu_ntt uses; inverse the
 * same with rho^-1, times n^-1.  points_out may alias points.  Refused with outputs untouched -- BBGPU_ERR_SIZE: n not a power of two, n < 2, n > 2^16,
 * batch < 1, batch * n > 2^20; BBGPU_ERR_ARG: a null pointer, any kind but BBGPU_FFT and BBGPU_IFFT (there is no coset transform on points), a point off the
 * curve or with a coordinate that is not canonical -- bbgpu_last_error() names the first such column and position.  The curve test runs on the HOST, in the
 * verdict the device entry and the twin share (a few products per point on up to 16 threads), so every refusal comes before a device is bound.
 * bbgpu_g1_recover, the decoder: the same `count` rows of every column are present -- a row that is missing lacks its commitment and all its proofs.  In
 * the notation of the bbgpu_kzg_recover_cells block with l = 1 and m = n = R: K the mu = n - count missing rows, g the coset generator of BBGPU_COSET_FFT,
 *   z_i = prod_{k in K} (rho^i - rho^k),   z'_i = prod_{k in K} (g rho^i - rho^k)       what k_recover_roots, k_recover_vanish and the batch inversion compute
 * at coset 1, once per call for all columns (hence n <= BBGPU_KZG_RECOVER_MAX_CELLS).  Per column:
 *   E_i = z_i * P_i on the present rows, infinity on the missing ones;   P = IFFT(E);   Q = FFT(g^j * P_j);   Q_i <- z'_i^-1 * Q_i;   D' = IFFT(Q);
 *   D_j = g^-j * D'_j;   points_out = FFT(D): ALL n points of the column in natural order
 * The verdict is exact, as in the field entry: the points are a codeword of degree < d iff coefficients [d, count) of every D are the point at infinity
 * (the group has prime order: a coefficient is at infinity iff the scalar decoder's is zero).  With count == d it is vacuous and says 1.  An inconsistent
 * column is still written and is a finding, not an error: the return value stays BBGPU_OK and the report names the first such column and its smallest
 * coefficient index not at infinity.  A coefficient in [count, n) that is not at infinity is BBGPU_ERR_HIP with a text of its own: no input can cause it.
 * Refused before a device is bound, outputs untouched -- BBGPU_ERR_SIZE: n not a power of two, n < 2, n > 2^16, degree_bound outside 1..n, count <
 * degree_bound, count > n, batch < 1, batch * n > 2^20; BBGPU_ERR_ARG: a null pointer, a row index >= n, a row listed twice, a point off the curve or not
 * canonical -- the message names the first offender.  Per-column row sets are bbgpu_g1_recover_each below (n <= 2^12).  Not here: n > 2^16 (the product
 * tree of kzg_recover_each.hip for the vanishing values), device-resident inputs and outputs, G2.
 * The kernels (csrc/g1_recover.hip).  A stage launch that does not fill the chip costs about the 0.9 ms one wave needs for its ladder, so a small decode
 * costs its count of ladder-bearing launches, not its count of points: 4 + 4 log2 n.
 *   k_g1_stage_cols  (n <= 64; from n = 128 on the drivers launch k_lagrange_stage, see the cost below) the butterfly of csrc/g1_stage.hpp (butterfly_slots<3>, unchanged) with (position, column, group) flattened into one lane index,
 *                    position-major: k_lagrange_stage takes the column from blockIdx.y and one lane per butterfly -- at R = 8 four live lanes in a wave of
 *                    64 and one wave per column.  Here consecutive lanes take consecutive (column, group) pairs at ONE position whenever batch x groups >=
 *                    64, so the twiddle and the skip of the ladder at position 0 stay wave-uniform; below that, consecutive positions as the existing
 *                    kernel.  Both entries use it; the existing group entries keep theirs and are not moved here
 *   four fused ladder passes, each "slot <- scalar * point" with the bit reversal of the NEXT transform folded in, so that no transform has a load or a
 *                    scale launch of its own: k_g1_load (n^-1 z_i) * P_i -> slot bitrev(i), infinity for missing rows; k_g1_scale three times: the coset
 *                    shift g^j, the division n^-1 / z'_i, the unshift g^-j.  A permuting pass in place is a race between a slot and its bit-reversed
 *                    partner: a call owns a SECOND SCRATCH and every pass reads one and writes the other (2 x 128 bytes per point).  The per-index
 *                    scalars come from four device tables k_g1_scalars makes once per call, plain canonical integers for the ladder
 *   k_g1_verdict     one workgroup per column between the unshift and the last transform (which consumes D in place): a min-reduction on chip over ZZ
 *                    != 0 in [d, count) and in [count, n), written without any atomic
 *   k_g1_finish      the affine form of every slot, one Fermat inversion per point as k_lagrange_finish and k_open_cosets_finish; a batch inversion over
 *                    the batch x n Z-coordinates was NOT built -- see the cost of the finish below
 * Resources (hipcc -Rpass-analysis=kernel-resource-usage, VGPRs / AGPRs / LDS bytes / waves per SIMD): k_g1_stage_cols
 * 231 / 0 / 0 / 2, k_g1_load 250 / 0 / 0 / 2, k_g1_scale 229 / 0 / 0 / 2 (the ladder's table fills the register file, as in k_lagrange_stage: 231), k_g1_scalars
 * 60 / 0 / 0 / 8 (50 before it took the per-column rows of bbgpu_g1_recover_each), k_g1_verdict 16 / 0 / 32 / 8, k_g1_finish 75 / 0 / 0 / 6; no scratch and
 * no spill in any.
 * Both entries run on context 0 under the library mutex.  A warm bbgpu_g1_recover at (n, d, missing, batch) = (8, 4, 4, 3) passes five allocations (the
 * lists; z, z', the tables and the roots; the points; the findings; the two scratches), three uploads (the lists, the findings' start, the points), two
 * read-backs (the findings, the points) and fifteen launch checks (roots + vanish; the inversion's two scans and its product; the tables; the load; four
 * transforms; three scale passes; the verdict; the finish); a warm bbgpu_g1_ntt two allocations, one upload, one read-back and three launch checks.  Every
 * site failed once through bbgpu_fault_inject returns BBGPU_ERR_HIP, leaves nothing the call allocated live, and the next call is bit-exact
 * (tests/test_gpu_g1_recover.py).  With bbgpu_set_timing(1), bbgpu_last_timing() of bbgpu_g1_recover: index 0 the vanishing values, 1 the load and the
 * first inverse transform, 2 shift, forward, divide, inverse, unshift and verdict, 3 the final transform and the finish, 4 the finish alone (a part of 3).
 * Cost on one MI355X (tools/g1_recover_bench.py, profiles/g1_recover.txt; wall ms per call, copies of the points across the link included, one process,
 * medians of 9 alternating pairs).  (a) k_g1_stage_cols against the parent's mapping (k_lagrange_stage, the column in blockIdx.y), the same forward
 * bbgpu_g1_ntt, new / old: (n, batch) = (8, 4096) 3.27 / 14.77; (64, 512) 6.34 / 7.53; (64, 8192) 22.07 / 40.04; (128, 256) 7.29 / 7.60; (128, 4096) 25.05 /
 * 26.90; (512, 65) 9.56 / 9.36; (2^16, 1) 17.32 / 17.04.  By the rule of the open-cosets block -- a median lower by more than the full range (max - min)
 * of either leg -- the new mapping wins (8, 4096) and (64, 8192), where the old one leaves lanes idle and launches a workgroup per column; at (64, 512) its
 * median is lower but one outlier of 11.6 ms widens the range past the gap; from n = 128 on every wave of either mapping is full, the medians lie within
 * 7 % of one another and inside the range, and at (2^16, 1) the two coincide as expected (1.6 %, the pool's +- 5 %).  So the drivers DISPATCH: k_g1_stage_cols
 * for n <= 64, k_lagrange_stage from n = 128 on (bbgpu_g1_set_stage_mapping forces either, for the bench).  (b) bbgpu_g1_recover against 4 + 4 log2 n times
 * the latency of one ladder-bearing launch, 1.28 ms in that run (the device time of k_g1_load with one ladder plus the one stage of n = 2, which is position 0
 * and runs none, at (2, 1): an upper estimate, two launches): (n, batch, missing) = (8, 65, 4) 13.2 ms wall, 12.9 device, 0.63 times 16 x 1.28; (512, 65, 256)
 * 37.0 wall, 36.0 device, 0.70 times; (4096, 16, 2048) 50.1 wall, 48.2 device, 0.72 times -- below one because stage 0 of every transform is position 0
 * throughout and runs no ladder (4 log2 n launches carry one, not 4 + 4 log2 n), and because slots at infinity skip theirs (half the load's at these shapes).
 * Nothing was tuned to that ratio.  Device times at (512, 65, 256): vanishing values 0.04, load + IFFT 8.4, shift .. verdict 19.3, FFT + finish 8.3.  The
 * finish kernel alone (bbgpu_last_timing index 4, a part of 3) takes 0.16 to 0.19 ms at 520 to 65536 points, under 2 % of any call: that is why one Fermat
 * inversion per point stayed and no batch inversion over the Z-coordinates was built.  (c) The alternative the decode replaces for a producer, at
 * (512, 65, 256) with d = 256: 37.3 ms for the 256 extension rows' commitments and proofs beside 261.7 ms for 16 calls of bbgpu_kzg_open_cosets_device at
 * (2^12, 64), batch 16, in the same process (which makes the proofs only, and needs the rows' data).  NOT timed: batch x n = 2^20, n = 2^16 in the decoder
 * (2^16 x 2^15 pair products for the vanishing values), columns with few rows missing, the host's curve test on its own, the host twins.
 * The host twins (csrc/host_g1_recover.hpp; plain loops over host_g1.hpp and g1_transform_host, a double-and-add per scalar, z and z' by direct
 * products; no HIP call, no lock, re-entrant) have the same refusals, the same canonical outputs and the same report: affine results are unique, so device
 * and twin agree bit for bit.  They are held to the scalar transform and the scalar decoder on multiples of the generator
 * (tests/test_g1_recover_host.py). */
typedef struct {
    uint32_t consistent;       /* 1: every column has coefficients [d, count) all at infinity (vacuous when count == d) */
    uint32_t first_bad_column; /* smallest b with a coefficient there that is not, else 0 */
    uint64_t first_bad_coeff;  /* its smallest such index, else 0 */
    uint64_t missing;          /* mu = n - count */
} bbgpu_g1_recover_report;
int bbgpu_g1_ntt(const uint64_t* points /* HOST, batch x n x 8 */, uint64_t* points_out /* HOST, batch x n x 8, may alias */, size_t n, int batch,
                 int kind /* BBGPU_FFT or BBGPU_IFFT */, void* hip_stream);
int bbgpu_host_g1_ntt(const uint64_t* points, uint64_t* points_out, size_t n, int batch, int kind);
int bbgpu_g1_recover(const uint32_t* row /* count, distinct, each < n, any order */, size_t count,
                     const uint64_t* points /* HOST, batch x count x 8: column b, listed row t */, size_t n, size_t degree_bound, int batch,
                     uint64_t* points_out /* HOST, batch x n x 8: ALL n points of every column, natural order */, bbgpu_g1_recover_report* report,
                     void* hip_stream);
int bbgpu_host_g1_recover(const uint32_t* row, size_t count, const uint64_t* points, size_t n, size_t degree_bound, int batch, uint64_t* points_out,
                          bbgpu_g1_recover_report* report);
/* the stage kernel both entries launch: 0 the dispatch described above (the default), 1 k_lagrange_stage with the column in blockIdx.y for every shape
 * (batch <= 65535, else BBGPU_ERR_SIZE from the entries), 2 k_g1_stage_cols for every shape -- for the comparison of tools/g1_recover_bench.py and the
 * tests; results are bit-identical.  BBGPU_ERR_ARG for any other value */
int bbgpu_g1_set_stage_mapping(int mapping);

/* ---- recover G1 codewords whose row sets differ  (one call for all columns: per-column vanishing values by direct pair products) ------
 * bbgpu_g1_recover above wants the same rows of every column.  A sampler that draws cells at random holds the proof pi_(r, c) for a DIFFERENT set of rows
 * r in every column c, and had to make one bbgpu_g1_recover call per distinct set -- each at the 4 + 4 log2 n ladder-bearing launches a call costs
 * whatever its batch.  bbgpu_g1_recover_each takes per-column row lists, as bbgpu_kzg_recover_cells_each does on the field side: column b lists count_b =
 * row_offsets[b + 1] - row_offsets[b] distinct rows with count_b >= d and misses the mu_b = n - count_b rows K_b; `points` holds row_offsets[batch] points
 * in the order of `row`.  Everything the block above fixes holds here: the point format, infinity as an ordinary input and output, complete additions,
 * the curve and canonicity test on the host before a device is bound, "a finding, not an error" for an inconsistent column, BBGPU_ERR_HIP with a text of
 * its own for a coefficient in [count_b, n) that is not at infinity, context 0 under the library mutex, the return after the last copy.  Column b has
 *   z_(b,i) = prod_{k in K_b} (rho^i - rho^k),   z'_(b,i) = prod_{k in K_b} (g rho^i - rho^k)
 * and the per-column decode is the one stated above with these; mu_b = 0 is legal and gives z = z' = 1.  first_bad_out, if given, receives per column the
 * smallest index in [d, count_b) whose coefficient is not at infinity, UINT64_MAX for none; the report names the first such column.  The device entry
 * writes report and first_bad_out only after its last copy has succeeded.
 * Refused before a device is bound, outputs untouched -- BBGPU_ERR_SIZE: n not a power of two, n < 2, n > BBGPU_G1_RECOVER_EACH_MAX_ROWS = 2^12,
 * degree_bound outside 1..n, batch < 1, batch * n > 2^20, for some b count_b < degree_bound or count_b > n; BBGPU_ERR_ARG: a null pointer (first_bad_out
 * may be NULL), row_offsets[0] != 0 or offsets that decrease, a row index >= n, a row listed twice within one column, a point off the curve or not
 * canonical -- bbgpu_last_error() names the first offender by column and position.
 * Why the cap is 2^12: the vanishing values are computed by DIRECT pair products, sum_b 2 mu_b n field products.  At n <= 2^12 and batch * n <= 2^20 that
 * is at most 2^32 products, about 29 ms at the 150 Gmul/s of csrc/fe_mont_gfx950.h, beside the same call's ladders -- expected to cost over a second when
 * the cap was chosen, 363 ms when measured (the cost below): the products are a small part either way.  At n = 2^16 they would be 2^36 at the same batch x n
 * (0.46 s), comparable with the ladders; that size needs the product tree of csrc/kzg_recover_each.hip.  Not here: n > 2^12 (the product tree), device-resident inputs
 * and outputs, G2.
 * The kernels (csrc/g1_recover.hip).  The transforms, the ladder passes, the verdict and the finish of bbgpu_g1_recover already run over a flattened
 * (position, column) index; what was per call and is per column here are the vanishing values and the per-index scalars:
 *   k_g1_roots       rho^k for every k < n, once per call: a table of n x 9 words (limb-major, Montgomery-261), square-and-multiply as k_recover_roots
 *   k_g1_vanish_cols the one compute-bound kernel of this entry: one lane per flattened (column, index) pair, index fastest; z_(b,i) as a Montgomery-261
 *                    multiplier and z'_(b,i) x 2^-5 in the memory format, exactly the forms kzg_recover_vanish writes, so that the batch inversion (over
 *                    batch x n elements) and the scalar tables follow unchanged.  A workgroup of 256 lanes stages the roots of missing rows in LDS tiles of
 *                    256 (9216 bytes, as k_recover_vanish); the missing lists go up in CSR form (offsets plus ascending rows).  For n >= 256 the workgroup
 *                    lies inside one column and walks that column's list tile by tile; for n < 256 it spans 256 / n whole columns, whose lists lie side by
 *                    side in the CSR array and together hold at most 256 roots (mu_b <= n - 1): one tile, of which every lane walks its own column's
 *                    sub-range.  Both products of a pair share the staged root, two accumulators per lane.  Columns in one wave may have different mu_b:
 *                    the tile loop and its two barriers depend on the workgroup alone, a lane's own range is a predicated inner loop, lanes past the end
 *                    of the grid have an empty range and write nothing -- no lane returns early
 *   per-column forms of the kernels above through added arguments whose zero or null value is bbgpu_g1_recover's behaviour: k_g1_scalars writes n^-1
 *                    z_(b,i) and n^-1 / z'_(b,i) as batch x n tables (g^j and g^-j stay n); k_g1_load takes slot_of per column (batch x n), the start of
 *                    the column's points (row_offsets[b] in place of b count) and the per-column table; k_g1_scale takes a table stride (the division
 *                    reads its column's row, shift and unshift stay shared); k_g1_verdict takes count_b from the offsets.  Stage kernels, dispatch and
 *                    k_g1_finish are unchanged, and bbgpu_g1_recover and bbgpu_g1_ntt are bit-identical with the same funnel counts
 * Resources (hipcc -Rpass-analysis=kernel-resource-usage, VGPRs / AGPRs / LDS bytes / waves per SIMD): k_g1_roots 39 / 0 / 0 / 8, k_g1_vanish_cols 82 / 0 /
 * 9216 / 5; the kernels that took arguments: k_g1_load 250 / 0 / 0 / 2, k_g1_scale 229 / 0 / 0 / 2 (both as before: the added index arithmetic is dead before
 * the ladder's table is live), k_g1_scalars 60 / 0 / 0 / 8 (50 before), k_g1_verdict 16 / 0 / 32 / 8; k_g1_stage_cols 231 and k_g1_finish 75 are untouched; no
 * scratch and no spill in any.
 * A warm call at (n, d, batch) = (8, 4, 3) with mu = 4, 3, 1 passes five allocations (the lists; z, z', the tables and the roots; the points; the
 * findings; the two scratches), three uploads (the lists -- slot_of, the row offsets and the CSR of the missing rows in one array --, the findings' start,
 * the points), two read-backs (the findings, the points) and fifteen launch checks (k_g1_roots with k_g1_vanish_cols; the inversion's two scans and its
 * product; the tables; the load; four transforms; three scale passes; the verdict; the finish).  Every site failed once through bbgpu_fault_inject returns
 * BBGPU_ERR_HIP, leaves nothing the call allocated live, and the next call is bit-exact (tests/test_gpu_g1_recover_each.py).  With bbgpu_set_timing(1),
 * bbgpu_last_timing(): index 0 the roots and k_g1_vanish_cols, 1 the load and the first inverse transform, 2 shift through verdict, 3 the last transform
 * and the finish, 4 the finish alone (a part of 3).
 * Cost on one MI355X (tools/g1_recover_each_bench.py, profiles/g1_recover_each.txt; wall ms per call, copies across the link included, one process,
 * medians of 9 alternating pairs; a median counts as lower only if it is lower by more than the full range of either leg; half the rows missing, d = n / 2).
 * (a) ONE call over `batch` columns with a different random half missing in each, against one bbgpu_g1_recover call per distinct set in the same process,
 * (n, batch): (8, 65), 45 distinct sets, 14.1 against 609.3 ms, 43 times; (64, 65), 65 sets, 27.8 against 1794.9, 65 times; (512, 65), 65 sets, 38.5 against
 * 2389.5, 62 times; (4096, 16), 16 sets, 54.0 against 791.4, 14.7 times -- every gap far beyond the range, and the ratio near the number of distinct sets as
 * launch counting predicts.  (b) The SAME set for all columns (every other row), this entry / bbgpu_g1_recover: (8, 65) 13.22 / 13.07 and (64, 65) 26.98 /
 * 26.95, both within the range; (512, 65) 37.64 / 37.08 and (4096, 16) 52.14 / 49.88, the same-set entry lower by more than the range: the price of the
 * per-column lists and tables, most of it the vanishing values -- 2.19 ms of device time at (4096, 16), where 65536 lanes each walk 2048 roots one after the
 * other and the same-set kernel spreads ONE column's n values over a wave per value.  (c) bbgpu_last_timing index 0 at (4096, 256) with a different random
 * half missing per column: 27.2 ms for sum_b 2 mu_b n = 2^32 products, 0.95 times their 28.6 ms at 150 Gmul/s; nothing was tuned to that ratio.  The same
 * call's ladder passes and transforms took 363 ms of device time (load + IFFT 92.3, shift .. verdict 190.9, FFT + finish 80.0): the direct products are 7 %
 * of the call at the largest shape the entry takes.  NOT timed: the host twin, the host's part of a call on its own (the curve test, the lists of missing
 * rows), the batch inversion over batch x n values on its own, columns that miss few rows beside columns that miss many in one call, n < 4096 at batch x n
 * = 2^20, a non-default stream.
 * The host twin (csrc/host_g1_recover.hpp g1_recover_each_host; plain loops, the one-column routine of g1_recover_host called once per column with that
 * column's set, z and z' by direct products; no HIP call, no lock, re-entrant) has the same refusals, the same canonical outputs, the same report and the
 * same first_bad_out.  It is held to the scalar decoder on multiples of the generator and to bbgpu_host_g1_recover where the sets agree
 * (tests/test_g1_recover_each_host.py). */
#define BBGPU_G1_RECOVER_EACH_MAX_ROWS (1u << 12)
typedef struct {
    uint32_t consistent;       /* 1: every column b has coefficients [d, count_b) all at infinity (vacuous where count_b == d) */
    uint32_t first_bad_column; /* smallest b that has not, else 0 */
    uint64_t first_bad_coeff;  /* its smallest such index, else 0 */
    uint64_t max_missing;      /* max over b of n - count_b */
} bbgpu_g1_recover_each_report;
int bbgpu_g1_recover_each(const uint32_t* row_offsets /* batch + 1, row_offsets[0] = 0, non-decreasing */,
                          const uint32_t* row /* row_offsets[batch]: column b owns row[row_offsets[b] .. row_offsets[b + 1]), distinct, each < n, any order */,
                          const uint64_t* points /* HOST, row_offsets[batch] x 8, in the order of `row` */, size_t n, size_t degree_bound, int batch,
                          uint64_t* points_out /* HOST, batch x n x 8: ALL n points of every column, natural order */,
                          uint64_t* first_bad_out /* HOST or NULL, batch: smallest index in [d, count_b) not at infinity, UINT64_MAX if none */,
                          bbgpu_g1_recover_each_report* report, void* hip_stream);
int bbgpu_host_g1_recover_each(const uint32_t* row_offsets, const uint32_t* row, const uint64_t* points, size_t n, size_t degree_bound, int batch,
                               uint64_t* points_out, uint64_t* first_bad_out, bbgpu_g1_recover_each_report* report);

/* ---- transform and recover the DATA of a 2-D layout down its columns  (a tile of whole columns decoded in LDS: one read, one write) ------
 * The blocks above work along a row on field elements (bbgpu_kzg_recover_cells, _each) and down a column on points (bbgpu_g1_ntt, bbgpu_g1_recover,
 * _each).  These entries are the fourth quadrant: down a column, on field elements.  A layout has k rows (polynomials), Reed-Solomon-extended column-wise
 * to rows = 2 k over the size-`rows` domain; a producer needs the extension rows' values, a sampler that holds enough rows of a column rebuilds the rest.
 * The matrix is DEVICE-resident and row-major: row r starts at element r * stride_elems, column j < width of row r is the 4-word element at (r *
 * stride_elems + j) * 4, in the reference's memory format (Montgomery-256); any representative below 2^256 is accepted, everything written is canonical.
 * Elements at [width, stride_elems) of every row are neither read nor written.  A codeword is a COLUMN: `rows` values, strided by the row length.
 * bbgpu_fr_ntt_columns_device transforms every column in place, natural order in and out, with rho = fr_root_of_unity(log2 rows) -- the root of bbgpu_ntt
 * and bbgpu_g1_ntt --, the inverse scaled by rows^-1.
 * bbgpu_fr_recover_columns_device: column j uses row set j mod sets.  Set s lists count_s = set_offsets[s + 1] - set_offsets[s] distinct PRESENT rows,
 * count_s >= d, and misses the mu_s = rows - count_s rows K_s.  sets = 1 is the whole-row case (a producer extending k rows, a node that holds complete
 * rows); sets = n / l is a sampler's: in a row, cell c holds entries c, c + m, c + 2 m, ... (m = n / l), so column j belongs to cell column j mod m.  Any
 * sets in 1..width is taken, a power of two or not.  Per column it is the decode the bbgpu_g1_recover block states, on scalars, with the z_(s,i) and
 * z'_(s,i) of bbgpu_g1_recover_each (set s in the place of column b):
 *   E_i = z_(s,i) v_i on the present rows, 0 on the missing ones;  P = IFFT(E);  Q = FFT(g^j P_j);  Q_i /= z'_(s,i);  D' = IFFT(Q);  D_j = g^-j D'_j;  V = FFT(D)
 * ONLY THE MISSING ROWS of each column are written, with V_i.  Present rows stay bit for bit as they were, also in an inconsistent column and also where
 * they held a non-canonical representative: the matrix is the caller's data and a finding must not destroy it.  A set that misses nothing is legal (z =
 * z' = 1): its columns get a verdict and no store.  The verdict is exact and is "a finding, not an error": a column is consistent iff coefficients [d,
 * count_s) of its D are zero (vacuous where count_s == d); the return value is BBGPU_OK, the report names the smallest inconsistent column and its smallest
 * such index, first_bad_out (if given) receives that index for every column, UINT32_MAX for none.  A nonzero coefficient in [count_s, rows) cannot come
 * from any input: BBGPU_ERR_HIP with a text of its own.  Report and first_bad_out are written only after the last copy has succeeded.
 * THE MAP IS LINEAR ACROSS ROWS: every output row is a fixed combination of the present rows, the same in every column of a set.  So the rows may equally
 * hold COEFFICIENTS: with sets = 1, recovering and then transforming each row equals transforming each row and then recovering, and the recovered rows of
 * coefficients are what bbgpu_kzg_open_cosets_device and an MSM read (tests/test_fr_columns_host.py, tests/test_gpu_fr_columns.py: commitments of the
 * recovered rows equal bbgpu_g1_recover's).
 * Refused before a device is bound, outputs untouched -- BBGPU_ERR_SIZE: rows not a power of two, rows < 2, rows > BBGPU_FR_COLUMNS_MAX_ROWS = 2^11 (the
 * NTT's sub-transform size: a whole column fits the 2048 LDS elements of a tile), width < 1, stride_elems < width, rows * width > 2^28, sets outside
 * 1..width, sets * rows > 2^20 (the size of the z tables, the cap bbgpu_g1_recover_each has), degree_bound outside 1..rows, for some s count_s <
 * degree_bound or count_s > rows; BBGPU_ERR_ARG: a null pointer (first_bad_out may be NULL), set_offsets[0] != 0 or offsets that decrease, a row index >=
 * rows, a row listed twice in one set -- bbgpu_last_error() names the first offender by set and position --, any kind but BBGPU_FFT and BBGPU_IFFT.  Not
 * here: rows > 2^11 (two passes), per-column degree bounds, G2.  Both device entries run on context 0 under the library mutex and return after the stream
 * has drained.
 * WHAT A FAILED CALL MAY HAVE WRITTEN: the decode is one launch, so a call that fails after it (a read-back, the BBGPU_ERR_HIP verdict above) may have
 * written MISSING rows, all or part; a call that fails before it has written nothing.  Present rows and the elements at [width, stride_elems) are never
 * written, by a failed call or any other (tests/test_gpu_fr_columns.py tests exactly that).  Report and first_bad_out stay as they were.
 * The kernels (csrc/fr_columns.hip; new HIP, the reference has no counterpart).  z and z' come from k_g1_roots and k_g1_vanish_cols (csrc/g1_recover.hip,
 * unchanged, "column" read as "set") and the batch inversion of csrc/poly.hip.
 *   k_fr_cols_tables  once per call: twiddles rho^k and rho^-k (rows / 2 each), g^j and g^-j (rows each), rows^-1 z_(s,i) and rows^-1 / z'_(s,i) (sets x
 *                     rows each) as Montgomery-261 MULTIPLIERS in 12-word entries -- field factors for the products below, not the plain integers a
 *                     ladder takes (k_g1_scalars); rows^-1 is folded into the two tables that meet an inverse transform, as there
 *   k_fr_cols_decode  the hot kernel.  A workgroup of 512 lanes owns a tile of C = 2048 / rows consecutive columns x all rows -- 2048 elements, nine limb
 *                     planes of 2048 words, 72 KiB of LDS, limb-major with the column fastest -- clipped at the end of the matrix (width need be no
 *                     multiple of C and no power of two).  Row segments of C x 32 bytes are read contiguously; missing rows are not read, their slots
 *                     start at zero.  Then everything happens in LDS: the scaling by rows^-1 z at the load, four radix-2 transforms with the three
 *                     pointwise passes between them, and the per-column verdict -- a zero test on the exact-limb product D_j for j >= d, the smallest
 *                     index per column by an LDS minimum that only a nonzero coefficient issues: an honest call issues no atomic, in LDS or in memory.
 *                     Then the store of the missing rows, canonical.  ONE read of the present elements and ONE write of the missing ones per call, no
 *                     scratch matrix.  No pass permutes: the inverse transforms run decimation in frequency (natural in, bit-reversed out), the forward
 *                     ones decimation in time (bit-reversed in, natural out), and the pointwise passes index their tables by bitrev.  Bank behaviour
 *                     (stated per access in the file): load, store and pointwise passes conflict-free; a stage of half h conflict-free where h C >= 64 and
 *                     2-way in the log2(64 / C) stages below that.  From rows = 1024 on a row segment (64 or 32 bytes) is narrower than a 128-byte line;
 *                     that is accepted, and its cost against a wider tile was not measured.  Lazy value bounds as csrc/ntt.hip keeps them, proved in the
 *                     file's header; decimation in frequency doubles the sums, so every fifth stage runs a reduce_value on half its outputs.
 *                     bbgpu_fr_ntt_columns_device is the same kernel text with the scaling, the verdict and the row skipping compiled out: one transform
 *                     (decimation in time behind a bit-reversed placement at the load), every row stored
 * Work: 4 (log2 rows) / 2 + 4 field products per element, 22 at rows = 512; a 512 x 2^16 matrix is 7.4e8 products, 4.9 ms at the 150 Gmul/s of
 * csrc/fe_mont_gfx950.h, against about 1 GiB of traffic.
 * Resources (hipcc -Rpass-analysis=kernel-resource-usage, VGPRs / AGPRs / LDS bytes / waves per SIMD): k_fr_cols_tables 41 / 0 / 0 / 8,
 * k_fr_cols_decode<true> 48 / 0 / 73,728 + 8 C dynamic (81,920 at C = 1024: two workgroups fill a CU's 163,840) / 8 by registers, 4 by LDS,
 * k_fr_cols_decode<false> (the transform) 45 / 0 / 73,728 dynamic / 8 by registers, 4 by LDS; no scratch and no spill in any.
 * A warm call with first_bad_out passes four allocations (the lists; z, z', the tables and the roots; the call's two findings; the per-column findings),
 * two uploads (the lists -- the CSR of the missing rows and the bits of the present ones in one array --, the findings' start), two read-backs (the two
 * findings, the per-column findings) and six launch checks (k_g1_roots with k_g1_vanish_cols; the inversion's two scans and its product; the tables; the
 * decode); without first_bad_out three allocations and one read-back.  bbgpu_fr_ntt_columns_device passes one allocation (the twiddles), no copy and two
 * launch checks.  Every site failed once through bbgpu_fault_inject returns BBGPU_ERR_HIP, leaves nothing the call allocated live, and the next call is
 * bit-exact (tests/test_gpu_fr_columns.py).  With bbgpu_set_timing(1), bbgpu_last_timing(): index 0 the roots, the vanishing values, their inversion and
 * the tables, index 1 the decode kernel.
 * Cost on one MI355X (tools/fr_recover_columns_bench.py, profiles/fr_recover_columns.txt; medians of 9 alternating pairs in one process; half the rows
 * missing, d = rows / 2): wall ms per call without first_bad_out; device ms of the decode kernel (bbgpu_last_timing index 1), beside (a) its own product count at 150 Gmul/s and (b)
 * the device time of four bbgpu_ntt_device_batch calls over the same elements as 64 transforms of rows x width / 64 -- existing code with more stages per
 * element, an upper reference and not a target.  (rows, width, sets): (512, 2^16, 1) 7.22 ms wall, decode 6.60 ms = 1.34 x (a) 4.92, 0.51 x (b) 13.00, the
 * vanishing values and tables 0.41; (512, 2^16, 1024) 12.03 wall -- 2^19 z values: 2.08 ms on the device and the host's lists --, decode 6.67 = 1.35 x (a), 0.52 x
 * (b) 12.89; (64, 2^16, 64) 0.94 wall, decode 0.600 = 1.34 x (a) 0.447, 0.50 x (b) 1.201; (8, 2^18, 1) 0.42 wall, decode 0.173 = 1.24 x (a) 0.140, 0.29 x (b)
 * 0.589; (2048, 2^12, 1) 3.33 wall, decode 2.07 = 1.43 x (a) 1.45, 0.74 x (b) 2.79 -- the one shape whose WALL time is above the four transforms' (2.83): its
 * vanishing values, 1024 roots walked by 2048 lanes, take 1.11 ms.  The decode runs at 0.70 to 0.81 of the multiplier's rate, the rest being the LDS round
 * trip of every stage, the 2-way conflicts stated above (rows = 2048: six of eleven stages) and the narrow row segments from rows = 1024 on, none of which
 * was measured on its own; nothing was tuned to these ratios.  NOT timed: the host twins, bbgpu_fr_ntt_columns_device on its own, rows >= 1024 against a
 * wider tile (two passes), widths that are no multiple of C, sets that miss different numbers of rows in one call, a call with first_bad_out, a non-default
 * stream.
 * The host twins (csrc/host_fr_columns.hpp; plain loops: gather a column, z and z' by direct products once per set, the one-polynomial decoder of
 * csrc/host_kzg_recover_cells.hpp over the radix-2 transform of csrc/host_fallback.hpp, scatter the missing rows; no HIP call, no lock, re-entrant) have
 * the same refusals, the same canonical outputs, the same report and the same first_bad_out.  They are held to Lagrange interpolation over Python integers,
 * to bbgpu_host_ntt column by column and to bbgpu_host_kzg_recover_cells_each at coset 1 (tests/test_fr_columns_host.py). */
#define BBGPU_FR_COLUMNS_MAX_ROWS (1u << 11)
int bbgpu_fr_ntt_columns_device(uint64_t* d_rows /* DEVICE, rows x stride_elems x 4 */, size_t rows, size_t width, size_t stride_elems,
                                int kind /* BBGPU_FFT or BBGPU_IFFT */, void* hip_stream);
int bbgpu_host_fr_ntt_columns(uint64_t* rows_mem /* HOST */, size_t rows, size_t width, size_t stride_elems, int kind);
typedef struct {
    uint32_t consistent;       /* 1: every column has coefficients [d, count_s) all zero (vacuous where count_s == d) */
    uint32_t first_bad_column; /* smallest such column, else 0 */
    uint64_t first_bad_coeff;  /* its smallest such index, else 0 */
    uint64_t max_missing;      /* max over sets of rows - count_s */
} bbgpu_fr_recover_columns_report;
int bbgpu_fr_recover_columns_device(const uint32_t* set_offsets /* HOST, sets + 1, set_offsets[0] = 0, non-decreasing */,
                                    const uint32_t* row /* HOST: set s owns row[set_offsets[s] .. set_offsets[s + 1]): its PRESENT rows, distinct, < rows, any order */,
                                    int sets, uint64_t* d_rows /* DEVICE */, size_t rows, size_t width, size_t stride_elems, size_t degree_bound,
                                    uint32_t* first_bad_out /* HOST or NULL, width entries: smallest nonzero index in [d, count_s), UINT32_MAX if none */,
                                    bbgpu_fr_recover_columns_report* report, void* hip_stream);
int bbgpu_host_fr_recover_columns(const uint32_t* set_offsets, const uint32_t* row, int sets, uint64_t* rows_mem /* HOST */, size_t rows, size_t width,
                                  size_t stride_elems, size_t degree_bound, uint32_t* first_bad_out, bbgpu_fr_recover_columns_report* report);

/* ---- is this proof valid?  (batches of proofs of one circuit: the per-proof scalars on the GPU, one pairing check) ------
 * waffle::Verifier::verify_proof (verifier.cpp:55-380) costs two pairings and a 20-point MSM per proof.  For a batch of proofs of ONE circuit the
 * per-proof part is what :55-355 computes -- six Keccak transcripts (challenge.hpp), the Lagrange evaluations (polynomial_arithmetic.cpp:594-626),
 * the linear terms (linearizer.hpp), t_eval, batch_evaluation and the widgets' scalars -- and the rest is folded with multipliers rho_j:
 *   A = sum_j rho_j (scalars on proof j's own nine points) + sum_k (sum_j rho_j s_jk) V_k     V_k: the key's points, then the generator (-batch_evaluation)
 *   B = sum_j rho_j (u_j PI_Z_OMEGA_j + PI_Z_j)
 *   pairing_ok = (e(A, G2) e(-B, x G2) == 1)                                                 one bbgpu_host_pairing_check of two pairs
 * over the proofs with status 0.  The batch is good iff every status is 0 and pairing_ok; the soundness error is about 2^-250 per check.
 * rho_j = Keccak-256(seed || j) with the top three bits cleared, derived and handed to the sums exactly as bbgpu_srs_check's multipliers are.
 * THE SEED MUST NOT BE KNOWN TO WHOEVER MADE THE PROOFS -- invalid proofs can be built to cancel for multipliers known in advance.  That is why
 * seed == NULL draws 32 bytes from the operating system (getrandom) and why the seed is reported only afterwards, so that a finding can be replayed.
 * A verifier handle holds n = 2^k, the widget set (the combinations bbgpu_plonk_circuit admits), the verification key exactly as
 * bbgpu_plonk_preprocess writes it (8 to 12 points, its order) and the transcript's x G2 (bbgpu_transcript_read_g2).  Create is host work: g2_x must be
 * on the twist, finite and of order r; every key point must carry the infinity flag (the commitment to a selector that is identically zero; it
 * contributes nothing, as the reference skips it) or lie on the curve.
 * status[j], a bit mask per proof of BBGPU_PLONK_PROOF_WORDS words (the reference's rules are verifier.cpp:59-102):
 *   BAD_POINT  Z_1, T_LO or PI_Z is not a finite point on the curve (g1::on_curve is false for infinity, group.hpp:536-551), OR one of W_L, W_R, W_O,
 *              T_MID, T_HI, PI_Z_OMEGA is finite and off the curve.  THE SECOND HALF IS STRICTER THAN THE REFERENCE, which silently leaves such a point
 *              out of its sum (:266-346; an off-curve PI_Z_OMEGA is still multiplied by u at :362) and then fails the pairing except with negligible
 *              probability: we reject outright.  One of those six WITH the infinity flag contributes nothing, exactly as the reference's skip does:
 *              honest proofs of a circuit with an identically zero wire are accepted (tests/golden/infinity_commitments.json).
 *   ZERO_EVAL  sigma_1_eval, sigma_2_eval or linear_eval is zero as fr::eq sees it: all four words zero (field.hpp:166-170).  The representative r is
 *              not zero there and not here: such a proof gets status 0 and is judged by the pairing (tests/golden/plonk_verify.json pins the case).
 * Evaluations and x coordinates may be any representative below 2^256, y coordinates any below 2^255 (bit 255 of y is the infinity flag, group.hpp:133-151:
 * a y with it set is never read as a finite coordinate); they are reduced before use, the transcript hashes what the reference hashes.
 * Return codes: BBGPU_OK means the check RAN; the verdict is in the report.  BBGPU_ERR_ARG: a null pointer, an unknown handle, an unknown flag or
 * widget bit, a bad key point or g2_x, count < 1; BBGPU_ERR_SIZE: n is not 2^k, count > BBGPU_PLONK_VERIFY_MAX_BATCH -- refused before a device is bound.
 * bbgpu_plonk_verify_batch has no host path, whatever the count (bbgpu_set_host_thresholds governs host-pointer MSMs only): kernel k_verify_terms does the
 * per-proof work, one proof per thread, k_verify_fold the sums over j of the shared terms (exact field additions in a fixed tree, no atomics), A and B are
 * two device MSMs in flight over transient tables the kernel wrote; the scalars never leave the device.  It runs on context 0 under the library mutex; its
 * buffers are library staging counted in bbgpu_memory_info.staging_bytes.  On any failure no MSM ticket is outstanding and the handle stays usable.
 * The report does not vary from run to run and, for the same seed, equals bbgpu_host_plonk_verify_batch's field for field, a and b included.
 * BBGPU_PLONK_VERIFY_LOCATE: after a failed pairing test the prefix length is bisected (prefix m passes iff every proof below m verifies): at most
 * ceil(log2 count) more rounds of one fold, two MSMs and one pairing check over the per-proof terms already computed, no new buffers.
 * Cost on one MI355X (tools/plonk_verify_bench.py, profiles/plonk_verify.txt; wall, one box, proofs of 2^16 gates): one call 2.12 ms at 256 proofs (upload,
 * k_verify_terms and status read-back 0.61, fold 0.02, the two MSMs 0.48, the host pairing check 1.02) and 3.72 ms at 2^14 (0.92 / 0.05 / 1.74 / 1.01):
 * 0.137 / 0.0084 / 0.00070 / 0.00023 ms per proof at 16 / 256 / 4096 / 2^14 proofs, against 0.165 / 0.0166 / 0.0062 for the host twin and about 0.8 ms for
 * the reference's verify_proof (a difference of two process walls of its driver, quartiles 0.4 .. 1.2 ms). */
#define BBGPU_PLONK_WIDGET_BOOL 1
#define BBGPU_PLONK_WIDGET_MIMC 2
#define BBGPU_PLONK_WIDGET_SEQUENTIAL 4
#define BBGPU_PLONK_VERIFY_BAD_POINT 1u
#define BBGPU_PLONK_VERIFY_ZERO_EVAL 2u
#define BBGPU_PLONK_VERIFY_LOCATE 1
#define BBGPU_PLONK_VERIFY_MAX_BATCH 16384
typedef struct {
    uint64_t count;             /* proofs in the batch */
    uint64_t bad_status;        /* proofs with status != 0 */
    uint64_t first_bad_status;  /* smallest such index, UINT64_MAX if none */
    uint32_t pairing_checked;   /* the pairing test ran */
    uint32_t pairing_ok;        /* e(A, G2) e(-B, x G2) == 1 over the proofs with status 0 */
    uint64_t first_bad_proof;   /* with BBGPU_PLONK_VERIFY_LOCATE and !pairing_ok: smallest j whose proof (status 0) does not verify, else UINT64_MAX */
    uint64_t seed[4];           /* the seed used (the caller's, or the one drawn), so that a finding can be replayed */
    uint64_t a[8], b[8];        /* A and B, affine (infinity flag honoured) */
} bbgpu_plonk_verify_report;
int bbgpu_plonk_verifier_create(size_t n, int widgets, const uint64_t vk[BBGPU_PLONK_VK_WORDS], const uint64_t g2_x[16]); /* handle >= 0; host work only */
int bbgpu_plonk_verifier_destroy(int verifier);
int bbgpu_plonk_verify_batch(int verifier, const uint64_t* proofs, size_t count, const uint64_t seed[4] /* NULL: OS randomness */, int flags,
                             uint32_t* status /* count */, bbgpu_plonk_verify_report* out);
/* DIAGNOSTIC (tools/plonk_verify_bench.py; not part of the verdict, one set of figures per process, overwritten by every call, zeros before the first):
 * wall ms of the last bbgpu_plonk_verify_batch or bbgpu_plonk_verify_multi, taken between the synchronisations the call makes anyway: total; upload, k_verify_terms and the read-back
 * of the statuses; k_verify_fold; the two MSMs; the host tail (pairing check, normalisations) -- with LOCATE summed over the rounds */
int bbgpu_plonk_verify_last_timing(double ms_out[5]);
/* the same definition on the host (csrc/host_plonk_verify.hpp), for a caller without a GPU or with one proof; no HIP call, no lock.  vk: as many points
 * as the widget set has (8 to 12) */
int bbgpu_host_plonk_verify_batch(size_t n, int widgets, const uint64_t* vk, const uint64_t g2_x[16], const uint64_t* proofs, size_t count,
                                  const uint64_t seed[4], int flags, uint32_t* status, bbgpu_plonk_verify_report* out);
/* PROOFS OF SEVERAL CIRCUITS IN ONE BATCH.  The fold is linear in the points and every circuit of one reference string meets the same x G2, so the
 * proofs of all circuits go into the same two sums and one product of two pairings.  Given verifier handles v_0 .. v_{G-1},
 * 1 <= G <= BBGPU_PLONK_VERIFY_MAX_CIRCUITS, `count` proofs in the caller's order and circuit[j] < G naming the handle whose circuit proof j claims:
 *   status[j]   as above: it depends on the proof alone
 *   rho_j     = Keccak-256(seed || j), top three bits cleared             j: the position in the caller's array
 *   A = sum_j rho_j (own scalars . own nine points of proof j, computed with n, root and widgets of circuit[j])
 *     + sum_c sum_k (sum over the j with circuit[j] = c of rho_j s_jk) V_{c,k}                  V_{c,.}: key c's points, then the generator
 *   B = sum_j rho_j (u_j PI_Z_OMEGA_j + PI_Z_j)
 *   pairing_ok = (e(A, G2) e(-B, x G2) == 1)
 * over the proofs with status 0; a key point at infinity has its scalar zeroed, per circuit.  A proof under the wrong label is a bad proof: it has
 * status 0 and fails the pairing.  BBGPU_PLONK_VERIFY_LOCATE bisects the prefix length over the caller's order exactly as above (prefix m passes iff every
 * proof below m verifies under its own label); the report is the same struct.  With G = 1 the definition IS bbgpu_plonk_verify_batch's and the report
 * equals that entry's field for field, a and b included.  The same handle may appear more than once in `verifiers`: legal, the same verdict (the sums
 * over a circuit's proofs are exact, how they are split shows in no result).
 * Refused before a device is bound -- BBGPU_ERR_ARG: a null pointer, num_verifiers < 1, an unknown handle, a circuit[j] >= num_verifiers (the error text
 * names j), handles whose g2_x differ (compared on the words the handle stores), an unknown flag, count < 1; BBGPU_ERR_SIZE: num_verifiers >
 * BBGPU_PLONK_VERIFY_MAX_CIRCUITS, count > BBGPU_PLONK_VERIFY_MAX_BATCH.
 * On the device (G > 1; with G = 1 the call IS bbgpu_plonk_verify_batch's, the same driver and kernels) each thread of k_verify_terms reads n, the widget
 * set and the domain's constants from its circuit's record (a table of G records the call uploads together with circuit[] and the shared rows, in one
 * copy), k_verify_fold sums slot k of circuit c in workgroup (k, c); a warm call passes
 * as many allocation / upload / read-back / launch checks and synchronises as often as bbgpu_plonk_verify_batch at the same count, whatever G.
 * bbgpu_plonk_verify_last_timing reports the last call of either GPU entry.  Cost: tools/plonk_verify_multi_bench.py, profiles/plonk_verify_multi.txt. */
#define BBGPU_PLONK_VERIFY_MAX_CIRCUITS 64
int bbgpu_plonk_verify_multi(const int* verifiers, int num_verifiers, const uint32_t* circuit /* count */, const uint64_t* proofs, size_t count,
                             const uint64_t seed[4] /* NULL: OS randomness */, int flags, uint32_t* status /* count */, bbgpu_plonk_verify_report* out);
/* the same on the host (csrc/host_plonk_verify.hpp): one key per circuit (n, widget set, vk of as many points as the set has), all under one g2_x;
 * for one seed the report equals bbgpu_plonk_verify_multi's field for field */
typedef struct {
    size_t n;
    int widgets;
    const uint64_t* vk;
} bbgpu_plonk_verify_key;
int bbgpu_host_plonk_verify_multi(const bbgpu_plonk_verify_key* keys, int num_keys, const uint64_t g2_x[16], const uint32_t* circuit /* count */,
                                  const uint64_t* proofs, size_t count, const uint64_t seed[4], int flags, uint32_t* status,
                                  bbgpu_plonk_verify_report* out);

/* ---- device self-test: known-answer entry points for the field and group layer ------------------------------------
 * One GPU lane per case runs the device arithmetic every kernel is built from (csrc/fe.hpp incl. the gfx950 asm products, csrc/g1.hpp);
 * operands and results in the reference's memory format, canonical.  What each op returns (a, b = the operands' residues):
 * field_impl_int128.tcc:72-137,149-263 / group.hpp:153-448 semantics. */
enum {
    BBGPU_SELFTEST_MUL = 0,        /* a b                         field::__mul          */
    BBGPU_SELFTEST_SQR = 1,        /* a^2                         field::__sqr          */
    BBGPU_SELFTEST_ADD = 2,        /* a + b                       field::__add          */
    BBGPU_SELFTEST_SUB = 3,        /* a - b                       field::__sub          */
    BBGPU_SELFTEST_NEG = 4,        /* -a                          field::__neg          */
    BBGPU_SELFTEST_MUL_ADD = 5,    /* a b + (a + b)(a - b)        two products, one Montgomery reduction */
    BBGPU_SELFTEST_MUL_SUB = 6,    /* a b - 2 a b                 the same with a negated operand */
    BBGPU_SELFTEST_LAZY_LIMBS = 7, /* 2a 3b                       unnormalised limbs at the multiplier's limit */
    BBGPU_SELFTEST_LAZY_WEAK = 8,  /* 4a (b - a)                  limbs beyond it: renormalised inside mul() */
    BBGPU_SELFTEST_LAZY_VALUE = 9, /* 28 a                        value bound at its maximum, 168 p < 2^261, through the multiplier */
    BBGPU_SELFTEST_REDUCE = 10,    /* 28 a                        the same through reduce_value() */
    BBGPU_SELFTEST_SQR_LAZY = 11,  /* (2a - b)^2 */
    BBGPU_SELFTEST_ZERO_TESTS = 12,/* limb 0: bit 0 = (a - b == 0), bit 1 = ((a - b) a == 0) */
    BBGPU_SELFTEST_MUL_ADDHI = 13, /* a b - a                     the product with a third operand added inside its reduction (in place; the mixed addition's P and R) */
    BBGPU_SELFTEST_SQR_ADDHI = 14, /* a^2 - (b + 2a)              the same for the squaring, addend with unnormalised limbs (the mixed addition's X3) */
    /* Raw-limb ops: the wide quotient-digit forms of csrc/fe.hpp themselves (32-bit digits 0..7, the top digit masked), result limbs as they come out.
     * A case is THREE consecutive rows (24 words) of a, b and out: a = the nine 32-bit limbs of operand a, then of c; b = limbs of b, then of d (a b + c d)
     * or of the addend e; out = the nine result limbs, then zeros.  n = 3 x cases. */
    BBGPU_SELFTEST_WIDE_MUL = 15,          /* REDC(a b) */
    BBGPU_SELFTEST_WIDE_SQR = 16,          /* REDC(a^2) */
    BBGPU_SELFTEST_WIDE_MUL2 = 17,         /* REDC(a b + c d) */
    BBGPU_SELFTEST_WIDE_MUL_IP = 18,       /* REDC(a b), in a's registers */
    BBGPU_SELFTEST_WIDE_MUL2_IP = 19,      /* REDC(a b + c d), in c's registers */
    BBGPU_SELFTEST_WIDE_MUL_ADDHI_IP = 20, /* REDC(a b) + e, in a's registers */
    BBGPU_SELFTEST_WIDE_SQR_ADDHI = 21,    /* REDC(a^2) + e */
    BBGPU_SELFTEST_WIDE_CHAIN = 22         /* case i: operand a of case i, then 255 in-place steps with the operands a of the cases after it (wrapping),
                                              cycling x y, x^2 + y, y x + x y, x y + y; operands: field values below 6 p with exact limbs */
};
enum {
    BBGPU_SELFTEST_G1_MADD = 0,      /* p + (q.x, q.y)                                             g1::mixed_add, group.hpp:219-322 */
    BBGPU_SELFTEST_G1_ADD = 1,       /* p + q                                                      g1::add, :324-448 */
    BBGPU_SELFTEST_G1_DBL = 2,       /* 2 p                                                        g1::dbl, :153-217 */
    BBGPU_SELFTEST_G1_DBL_AFFINE = 3,/* 2 p for an affine p (the P + P branch of the mixed addition) */
    BBGPU_SELFTEST_G1_MADD_NEG = 4,  /* p - (q.x, q.y): the conditionally negated operand the bucket accumulation feeds (group_impl_asm.tcc:71-153) */
    BBGPU_SELFTEST_G1_QUAD_ADD = 5,  /* p + q by the four-lanes-per-point addition of the bucket reduction (csrc/g1_quad.hpp) */
    BBGPU_SELFTEST_G1_MADD_IP = 6,   /* p +- (q.x, q.y) as ONE TRIP of the bucket accumulation does it: q limb 8 != 0 = negative digit; the operand packed as a
                                        table row and read back signed, the start branch for an infinite p, else madd_ip with infinity as a flag.  A flag that
                                        disagrees with the accumulator afterwards gives all-ones in the 16 output limbs */
    BBGPU_SELFTEST_G1_MADD_IP_CHAIN = 7 /* out[i] = sum of count_i signed operands of the ring q[begin_i .. end_i) from q[start_i] on, wrapping, folded that way from
                                        an infinite start; p row i carries start_i, count_i, begin_i, end_i in limbs 0-3 (n <= 4096, count <= 4096, end <= n; out
                                        of range: all-ones).  The caller gives each lane of a wave a sequence of its own, or the same one with different counts */
};
/* field: 0 = fq, 1 = fr; a, b, out: n x 4 limbs */
int bbgpu_selftest_field(int field, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out);
/* p, q: n x 12 limbs (Jacobian {x, y, z}, infinity flag honoured); out: n x 16 limbs {X, Y, ZZ, ZZZ} with x = X / ZZ, y = Y / ZZZ,
 * ZZ = 0 for infinity (the kernels' extended-Jacobian form; the caller normalises) */
int bbgpu_selftest_g1(int op, const uint64_t* p, const uint64_t* q, size_t n, uint64_t* out);

/* the endomorphism split of csrc/srs_update.hip, on the device (on_device != 0) or the same function on the host: k: n x 4 limbs, plain integers;
 * out: n x 6 limbs {|k1| lo, hi, |k2| lo, hi, flags, 0} with k = +-k1 - lambda (+-k2) (mod r); flags bit 0: k1 negative, bit 1: k2 negative, bit 2: a
 * magnitude does not fit 128 bits (never).  Where both signs are positive the magnitudes are host_wnaf.hpp's split (tests/golden/endo_wnaf.json). */
int bbgpu_selftest_endo_split(int on_device, const uint64_t* k, size_t n, uint64_t* out);

/* One round kernel of the PLONK prover (csrc/poly.hip) on its own, through the host function the prover itself calls (poly.h: *_lanes, scan_lanes,
 * evaluate_lanes) with a lane table of the entry's own: records, challenge-dependent constants and grids are made by the product's code.  Host pointers
 * in and out; the entry allocates, uploads, synchronises, downloads and frees.  Every vector is LANE-MAJOR: lane l's elements follow lane l - 1's, 4 limbs
 * each, in the reference's memory format (any value below 2^256 is a legal input; outputs are canonical).  `len` is the kernel's own length; the per-lane
 * length of each vector is given below in units of len.  consts: Fr values in memory form, CANONICAL (the prover's challenges are), `lanes` x k of them
 * (lane-major) unless stated.  Fresh outputs are preset to all-ones, so an element a kernel leaves out cannot pass for a field value.
 *   kernel             len   params                          in (per-lane length)                                   consts per lane        out
 *   Z_TERMS            n     -                               w_l w_r w_o s1 s2 s3 (n)                               beta gamma             num den (n)
 *   QUOT_LARGE         4n    -                               wl wr wo s1 s2 s3 zf (len)                             beta gamma             q (len)
 *   QUOT_MID           2n    -                               zf wl wr wo (2 len), l1 qm ql qr qo qc (len)           alpha alpha_base       q (len)
 *   QUOT_SEQ           2n    -                               wo (2 len), q_o_next (len), q (len)                    c                      q (len)
 *   QUOT_BOOL          2n    -                               wl wr wo (2 len), q_bl q_br q_bo (len), q (len)        c_l c_r c_o            q (len)
 *   QUOT_MIMC          4n    -                               wl wr wo q_sel q_coef q (len)                          alpha_base alpha_step  q (len)
 *   LINCOMB            n     count (1..12), has_addend       p_0 .. p_(count-1) [addend] (len)                      c_0 .. c_(count-1)     out (len)
 *   MUL2C              n     -                               a b (len)                                              c                      out (len)
 *   SIGMA_PREPARE      n     n_dst (>= len)                  sigma w (len)                                          gamma                  dst (n_dst)
 *   COPY_PAD           n_src n_dst (>= len), scaled          src (len)                                              c if scaled, else none dst (n_dst)
 *   ADD_INPLACE        n     stride_a, stride_b (>= len)     a (stride_a), b (stride_b)                             -                      a (stride_a)
 *   DIVIDE_VANISHING   N     log2(N / n) (0..2), stride >= N c (stride)                                             -                      c (stride)
 *   SCAN               n     mode (0 products, 1 Horner),    in (len); `lanes` is the number of jobs                z (mode 1 only)        [out (len)] [total (1)]
 *                            flags: 1 reverse, 2 inclusive,
 *                            4 an output vector, 8 a total
 *   EVALUATE           n     nz (1..16), zidx[0..lanes)      coefficients (len); `lanes` is the number of jobs      nz points IN ALL       result (1)
 * BBGPU_ERR_ARG, before a device is touched: an unknown kernel, lanes outside 1..16, len 0 or lanes x (the longest vector) above 2^22, a length that is
 * no power of two where the kernel masks indices or takes a root of unity (Z_TERMS, the QUOT_* kernels, DIVIDE_VANISHING), a wrong number of vectors,
 * parameters or constants, a null pointer, a constant that is not below r, a parameter outside the range above (a destination or stride shorter than len,
 * a zidx outside nz, a SCAN that asks for neither output).  All lanes of a call have one length: the kernels take their grid from lane 0. */
enum {
    BBGPU_SELFTEST_PLONK_Z_TERMS = 0,
    BBGPU_SELFTEST_PLONK_QUOT_LARGE = 1,
    BBGPU_SELFTEST_PLONK_QUOT_MID = 2,
    BBGPU_SELFTEST_PLONK_QUOT_SEQ = 3,
    BBGPU_SELFTEST_PLONK_QUOT_BOOL = 4,
    BBGPU_SELFTEST_PLONK_QUOT_MIMC = 5,
    BBGPU_SELFTEST_PLONK_LINCOMB = 6,
    BBGPU_SELFTEST_PLONK_MUL2C = 7,
    BBGPU_SELFTEST_PLONK_SIGMA_PREPARE = 8,
    BBGPU_SELFTEST_PLONK_COPY_PAD = 9,
    BBGPU_SELFTEST_PLONK_ADD_INPLACE = 10,
    BBGPU_SELFTEST_PLONK_DIVIDE_VANISHING = 11,
    BBGPU_SELFTEST_PLONK_SCAN = 12,
    BBGPU_SELFTEST_PLONK_EVALUATE = 13
};
int bbgpu_selftest_plonk_round(int kernel, int lanes, size_t len, const uint32_t* params, int num_params, const uint64_t* const* in, int num_in,
                               const uint64_t* consts, size_t num_consts, uint64_t* const* out, int num_out);

/* ---- instrumentation (bench.py) ---------------------------------------------------------------------------------
 * Device time in milliseconds of the kernels launched by the most recent bbgpu_*_device call on this thread, measured
 * with hipEvents on the stream the kernels ran on.  index: 0 = total, then per stage: 1 digits, 2 sort, 3 accumulation,
 * 4 merge, 5 row/column sums, 6 final sums, 7 accumulation without the time it sat queued behind the previous MSM's accumulation. */
int bbgpu_last_timing(float* ms_out, int max_entries);
void bbgpu_set_timing(int level); /* 0 off; 1 an event after every stage (adds ~0.08 ms of marker latency to a pipelined 2^20 step); 2 only
                                     the pair around the accumulation (indices 3 and 7 are filled): what bench.py's timed region uses */

#ifdef __cplusplus
}
#endif
#endif /* BBGPU_H */
