// capi.hip -- the C-ABI of libbbgpu.so (include/bbgpu.h): context, SRS registry, host<->device staging.
// One process drives one GPU (bbgpu_init(device)), or several device contexts (bbgpu_init_devices) over which the host-pointer MSMs are split; all
// entry points are serialised by one mutex, which also makes the reference's concurrent pippenger() calls from an OpenMP region
// (scalar_multiplication.cpp:731-738) safe.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <optional>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <atomic>
#include <condition_variable>
#include <exception>
#include <functional>
#include <thread>
#include <unordered_map>
#include <vector>

#include "bbgpu_internal.h"
#include "host_g1.hpp"
#include "host_g2.hpp"
#include "host_small.hpp"
#include "host_fallback.hpp"
#include "host_copy_pool.hpp"
#include "host_pairing.hpp"
#include "host_srs_check.hpp"
#include "host_srs_update.hpp"
#include "host_srs_lagrange.hpp"
#include "host_kzg_check.hpp"
#include "host_kzg_check_batch.hpp"
#include "host_kzg_check_cells.hpp"
#include "host_lagrange_open.hpp"
#include "host_srs_lagrange_check.hpp"
#include "host_kzg_open_all.hpp"
#include "host_kzg_open_cosets.hpp"
#include "host_kzg_recover_cells.hpp"
#include "host_kzg_recover_each.hpp"
#include "host_g1_recover.hpp"
#include "host_fr_columns.hpp"
#include "host_plonk_verify.hpp"
#include "multi_plan.hpp"
#include "poly.h"

namespace bbgpu {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- the funnels of bbgpu_internal.h: allocation accounting + fault injection ---------------------------------------------------------------
// BBGPU_FAIL_AT (read once, when the first funnel is reached) or bbgpu_fault_inject(): "<kind>:<k>" with kind in alloc | h2d | d2h | launch makes the
// k-th call (k = 0: the next one) of that kind fail ONCE with the error a real failure of that kind returns, without touching the device; the
// call after it works again.  Counters restart whenever a spec is set.  Host-side only: no kernel reads any of it.
namespace {
enum FaultKind { F_ALLOC = 0, F_H2D = 1, F_D2H = 2, F_LAUNCH = 3, F_KINDS = 4 };
struct FaultState {
    std::mutex mu;
    std::atomic<int> armed_kind{ -1 };   // -1: nothing armed (the one load every funnel call pays)
    uint64_t fail_at = 0;
    std::atomic<uint64_t> calls[F_KINDS] = {};
    std::atomic<uint64_t> fired{ 0 }, absorbed{ 0 };
    std::unordered_map<void*, size_t> live; // device allocations of the library that are live now
    uint64_t live_bytes = 0;
    bool env_read = false;
};
FaultState& fault()
{
    static FaultState* f = new FaultState(); // never destroyed: funnels run during static destruction of other objects too
    return *f;
}
int fault_parse(const char* spec, int* kind, uint64_t* at)
{
    static const char* names[F_KINDS] = { "alloc", "h2d", "d2h", "launch" };
    if (!spec || !*spec) { *kind = -1; return 0; }
    for (int k = 0; k < F_KINDS; k++) {
        const size_t len = strlen(names[k]);
        if (!strncmp(spec, names[k], len) && spec[len] == ':') {
            char* end = nullptr;
            *at = strtoull(spec + len + 1, &end, 0);
            if (end == spec + len + 1 || *end) return -1;
            *kind = k;
            return 0;
        }
    }
    return -1;
}
int fault_set(const char* spec)
{
    FaultState& F = fault();
    int kind = -1;
    uint64_t at = 0;
    if (fault_parse(spec, &kind, &at)) return -1;
    std::lock_guard<std::mutex> lk(F.mu);
    F.env_read = true; // an explicit spec overrides the environment
    for (auto& c : F.calls) c.store(0);
    F.fired.store(0);
    F.absorbed.store(0);
    F.fail_at = at;
    F.armed_kind.store(kind);
    return 0;
}
// true: this call is the one to fail
bool fault_hit(FaultKind kind)
{
    FaultState& F = fault();
    if (!F.env_read) {
        std::lock_guard<std::mutex> lk(F.mu);
        if (!F.env_read) {
            F.env_read = true;
            int k = -1;
            uint64_t at = 0;
            const char* e = getenv("BBGPU_FAIL_AT"); // testing: "alloc:k" / "h2d:k" / "d2h:k" / "launch:k" makes the k-th such call of the process fail once (include/bbgpu.h, bbgpu_fault_inject)
            if (e && fault_parse(e, &k, &at) == 0 && k >= 0) {
                F.fail_at = at;
                F.armed_kind.store(k);
            } else if (e && *e) {
                fprintf(stderr, "bbgpu: BBGPU_FAIL_AT=%s not understood (alloc:k | h2d:k | d2h:k | launch:k)\n", e);
            }
        }
    }
    const uint64_t n = F.calls[kind].fetch_add(1);
    if (F.armed_kind.load(std::memory_order_relaxed) != (int)kind) return false;
    std::lock_guard<std::mutex> lk(F.mu);
    if (F.armed_kind.load() != (int)kind || n != F.fail_at) return false;
    F.armed_kind.store(-1); // one shot
    F.fired.fetch_add(1);
    return true;
}
} // namespace

hipError_t dev_malloc(void** p, size_t bytes)
{
    if (fault_hit(F_ALLOC)) {
        *p = nullptr;
        set_error("hipMalloc(%zu bytes) -> %s [injected by BBGPU_FAIL_AT]", bytes, hipGetErrorString(hipErrorOutOfMemory));
        return hipErrorOutOfMemory;
    }
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess && *p) {
        FaultState& F = fault();
        std::lock_guard<std::mutex> lk(F.mu);
        F.live[*p] = bytes;
        F.live_bytes += bytes;
    }
    return e;
}
hipError_t dev_free(void* p)
{
    if (!p) return hipSuccess;
    {
        FaultState& F = fault();
        std::lock_guard<std::mutex> lk(F.mu);
        auto it = F.live.find(p);
        if (it != F.live.end()) {
            F.live_bytes -= it->second;
            F.live.erase(it);
        }
    }
    return hipFree(p);
}
hipError_t h2d_async(void* dst, const void* src, size_t bytes, hipStream_t st)
{
    if (fault_hit(F_H2D)) {
        set_error("hipMemcpyAsync(host to device, %zu bytes) -> %s [injected by BBGPU_FAIL_AT]", bytes, hipGetErrorString(hipErrorInvalidValue));
        return hipErrorInvalidValue;
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st);
}
hipError_t d2h_async(void* dst, const void* src, size_t bytes, hipStream_t st)
{
    if (fault_hit(F_D2H)) {
        set_error("hipMemcpyAsync(device to host, %zu bytes) -> %s [injected by BBGPU_FAIL_AT]", bytes, hipGetErrorString(hipErrorInvalidValue));
        return hipErrorInvalidValue;
    }
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
}
hipError_t launch_check()
{
    const hipError_t e = hipGetLastError(); // a real failure is reported (and cleared) first
    if (e != hipSuccess) return e;
    if (fault_hit(F_LAUNCH)) {
        set_error("kernel launch -> %s [injected by BBGPU_FAIL_AT]", hipGetErrorString(hipErrorLaunchFailure));
        return hipErrorLaunchFailure;
    }
    return hipSuccess;
}
void fault_absorbed() { fault().absorbed.fetch_add(1); }

namespace {

struct SrsEntry {
    const uint64_t* host_ptr; // may be null for device-generated tables
    size_t n;
    uint32_t* d_srs;
    bool live;
    // Pre-shifted window tables, one per SEGMENT of at most 2^24 / W points (the sorted entries carry a 24-bit table row: 2^20 points at 15 windows).
    // A larger SRS keeps several segments of equal length and an MSM over it runs as one piece per segment it touches, the piece sums added on
    // the host -- the point-range split of scalar_multiplication.cpp:703-738 inside one GPU.  Empty: no tables (per-window bucket sets).
    struct TabSeg {
        size_t first = 0, n = 0;          // points [first, first + n) of the entry
        uint32_t* d_tab = nullptr;       // [tab_W][n] rows of 64 bytes: the address window 0 has (or would have)
        uint32_t* d_tab_alloc = nullptr; // the allocation itself: starts at window tab_wb when only a share of the windows is kept
    };
    std::vector<TabSeg> segs;
    bool has_tab() const { return !segs.empty(); }
    int tab_c = 0, tab_W = 0, tab_wb = 0, tab_we = 0; // windows [tab_wb, tab_we) are resident (the same for every segment)
    // Address-keyed lookups are only trusted after a CONTENT check: one 64-bit hash per base point (the even table entry the kernels
    // read), taken when the table was uploaded.  A lookup re-hashes the first, the last and up to 14 evenly spaced rows of the range
    // the caller passed (it never touches host memory outside that range: the old table may have been freed) and compares.
    std::vector<uint64_t> row_hash;
    bool auto_registered = false; // created by a host-pointer MSM on first sight: evictable (stale contents, overlap, LRU under the byte cap)
    uint64_t last_use = 0;
    size_t bytes = 0; // device bytes held (points + window tables)
    bool handle_exposed = false; // the index was returned to a caller as a handle: the slot is never reused for another table
    uint64_t check_phase = 0;    // rotates the rows a content check samples (contents_match)
    bool stale_for_host = false; // exact mode found the caller's memory changed under an EXPLICITLY registered table: host-pointer calls no longer use it (the handle stays valid)
    bool validate_full = false;  // EXACT mode (bbgpu_srs_set_validate / BBGPU_SRS_VALIDATE=full): every host-pointer MSM re-hashes the whole range it uses
};

// eight independent multiplications (odd multipliers: a change of one limb always changes the sum) instead of a dependent chain: the full content
// check of BBGPU_SRS_VALIDATE=full hashes every row of the range on every call and must run at memory speed
inline uint64_t hash_row(const uint64_t* row8)
{
    static const uint64_t M[8] = { 0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL, 0x94d049bb133111ebULL, 0xd6e8feb86659fd93ULL,
                                   0xca5a826395121157ULL, 0xff51afd7ed558ccdULL, 0xc4ceb9fe1a85ec53ULL, 0x2545f4914f6cdd1dULL };
    uint64_t h = 0;
    for (int i = 0; i < 8; i++) h += (row8[i] ^ M[(i + 3) & 7]) * M[i];
    h ^= h >> 31;
    return h * 0x9e3779b97f4a7c15ULL;
}

struct Context {
    bool ready = false;
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<SrsEntry> srs;
    static constexpr int NSLOT = 8; // asynchronous MSMs in flight (each with its own workspace and stream; workspaces are allocated on first use)
    MsmSlot slot[NSLOT];
    int next_slot = 0;
    uint64_t* d_stage = nullptr; // scalars / coefficients staging
    size_t stage_cap = 0;
    uint64_t* d_stage2 = nullptr; // second scalar staging buffer (pipelined batches)
    size_t stage2_cap = 0;
    uint64_t* d_scratch = nullptr; // NTT scratch
    size_t scratch_cap = 0;
    uint64_t* d_small_tab = nullptr; // a small point table that is used once (raw upload + working form): kept, so that such a call allocates and frees nothing
    size_t small_tab_cap = 0;
    uint64_t* d_srs_check = nullptr; // bbgpu_srs_check: the curve findings (first 64 bytes), then the n - 1 multipliers of 32 bytes
    size_t srs_check_cap = 0;
    uint64_t* d_verify = nullptr; // bbgpu_plonk_verify_batch: the proofs, the rows and scalars of the two sums, the shared terms, the statuses
    size_t verify_cap = 0;
    uint64_t* d_kzg_check = nullptr; // bbgpu_kzg_check_*: the caller's arrays, the rows and scalars of the two sums, the terms, the partial sums, the findings
    size_t kzg_check_cap = 0;
    int timing = 0; // 0 off, 1 every stage, 2 the accumulation only (bbgpu_set_timing)
    bool precompute = true; // build window tables for registered SRS (bbgpu_set_precompute)
    uint64_t use_clock = 0;  // LRU clock of the SRS cache
    size_t srs_cache_cap = (size_t)16 << 30; // device bytes the auto-registered tables may hold together (BBGPU_SRS_CACHE_BYTES)
    bool srs_validate_full = false;          // default of SrsEntry::validate_full for tables registered from now on
    // SURVEY 8b "small sizes": host-pointer MSMs of at most host_msm_max points against tables that are not resident, and host-buffer
    // transforms of at most host_ntt_max elements, are answered on the host (host_small.hpp); bbgpu_set_host_thresholds / BBGPU_HOST_MSM_MAX /
    // BBGPU_HOST_NTT_MAX.  Defaults from tools/small_sizes.py on MI355X + EPYC 9575F: MSM n = 4 / 20 / 32 / 64 host 0.16 / 0.31 / 0.41 /
    // 0.73 ms against 0.35-0.37 ms through the kernels (crossover near 24 points); transforms n = 4 / 16 / 64 host 9 / 13 / 68 us against 37-43 us
    int host_msm_max = 24;
    int host_ntt_max = 16;
    bool host_env_read = false;
    int share_rank = 0, share_world = 1; // window share of the tables built from now on (bbgpu_set_table_share)
    int point_world = 1;                 // tables built from now on hold 1 / point_world of the points of a larger MSM (bbgpu_set_point_share)
    hipEvent_t helper_dep[NSLOT] = {};   // orders a helper slot's stream behind the caller's stream (issue_ticket)
    // Workspaces shared by every caller (NTT scratch, polynomial temporaries): users on different streams are chained by this event
    hipEvent_t shared_done = nullptr;
    hipStream_t shared_last = nullptr;
    bool shared_used = false;
    poly::Scratch poly_scratch; // workspace of the resident polynomial helpers
    uint64_t* d_poly_tmp = nullptr;
    size_t poly_tmp_cap = 0;
    MsmTiming last;
    // pinned staging for the callers' host buffers (host_to_device / device_to_host_sync)
    // 8 x 1 MiB (round 3: 2 x 4 MiB): the first chunk reaches the link after 1 MiB of CPU copy instead of 4, and up to seven chunks are queued behind
    // it -- bbgpu_ntt at 2^18 (8 MiB each way) 0.651 -> 0.617 ms, the reference prover on the shim level within its own noise (tools/stage_chunk_ab.sh)
    static constexpr size_t HOST_CHUNK = (size_t)1 << 20; // bytes per pinned staging buffer
    static constexpr int HOST_RING = 8;                   // staging buffers (a ring: the CPU copies run ahead of the DMA of the chunks before them)
    size_t host_chunk = HOST_CHUNK;                       // bytes of a buffer actually used per chunk (BBGPU_STAGE_CHUNK_BYTES <= HOST_CHUNK)
    void* h_stage[HOST_RING] = {};
    hipEvent_t h_stage_free[HOST_RING] = {};
    unsigned h_stage_next = 0;
    size_t host_stage_max = (size_t)8 << 20; // BBGPU_STAGE_MAX_BYTES: larger buffers are handed to hipMemcpyAsync as they are
    bool stage_env_read = false;             // the two staging variables above have been read (once per context)
    host::CopyPool copy_pool; // CPU copies into / out of the pinned staging buffers (host_copy_pool.hpp); also hashes point tables (exact cache mode)
    AccRing acc_ring;         // "accumulation ended" events of this context's timed MSMs (msm.hip)
    // Set while this context runs its slice of a split host-pointer MSM: the number of points of the WHOLE call, whose window size the slice's tables
    // take (as bbgpu_set_point_share does, without touching the caller's share settings).  0 otherwise.
    size_t slice_of_n = 0;
    std::recursive_mutex own_mu; // the lock of contexts 1 .. (context 0's is g_mu): its staging buffers, copy pool, initialisation
};

// Device contexts (bbgpu_init_devices).  Context 0 is what every entry point works on; the others exist only for the split host-pointer MSMs, each
// driven by a persistent worker thread of its own (MultiWorker below).  A thread's CURRENT context is context 0 unless it is such a worker.
// g_mu is the entry lock of the public API and the lock of context 0.  A split call holds it while the workers run: so the helpers a worker calls
// (ensure_init, host_to_device, device_to_host_sync, host_stage_release) take the lock of the CURRENT context, never g_mu itself.  While g_mu is free
// every worker is idle, so an entry point that holds it may read any context.
std::recursive_mutex g_mu;
Context g_ctxs[BBGPU_MAX_CONTEXTS];
int g_num_ctx = 1; // contexts bound by bbgpu_init_devices (1: bbgpu_init, or nothing bound yet)
thread_local int t_ctx = 0;
inline Context& ctx() { return g_ctxs[t_ctx]; }
inline std::recursive_mutex& ctx_lock() { return t_ctx == 0 ? g_mu : ctx().own_mu; }

void read_host_env()
{
    // the staging knobs are read once per context whatever else happened; the two thresholds only while bbgpu_set_host_thresholds() has not set them
    // (round 5: that call used to switch off the reading of ALL four variables).  Every context reads the same variables, so all agree.
    if (!ctx().host_env_read) {
        ctx().host_env_read = true;
        if (const char* e = getenv("BBGPU_HOST_MSM_MAX")) ctx().host_msm_max = atoi(e);
        if (const char* e = getenv("BBGPU_HOST_NTT_MAX")) ctx().host_ntt_max = std::min(64, atoi(e));
    }
    if (ctx().stage_env_read) return;
    ctx().stage_env_read = true;
    if (const char* e = getenv("BBGPU_STAGE_MAX_BYTES")) ctx().host_stage_max = (size_t)strtoull(e, nullptr, 0);
    if (const char* e = getenv("BBGPU_STAGE_CHUNK_BYTES")) ctx().host_chunk = std::min(Context::HOST_CHUNK, std::max((size_t)64 << 10, (size_t)strtoull(e, nullptr, 0))); // testing hook: the chunk size of the staging copies
}

int hip_device_count()
{
    // asked once per process: without a device every call would repeat the runtime's probe of the machine (~10 ms each; the shim's host
    // answers would be paced by it)
    static const int cnt = [] { int c = 0; return hipGetDeviceCount(&c) == hipSuccess ? c : 0; }();
    return cnt;
}

int ensure_init()
{
    std::lock_guard<std::recursive_mutex> lk(ctx_lock());
    if (ctx().ready) {
        // HIP's current device is PER THREAD (device 0 in a fresh one): a caller's worker thread -- the reference's OpenMP threads around pippenger(),
        // bench.py's issuing thread on rank r > 0 -- must allocate and launch on the device this process is bound to, not on device 0
        static thread_local int bound_device = -1;
        if (bound_device != ctx().device) {
            HIPCHK(hipSetDevice(ctx().device));
            bound_device = ctx().device;
        }
        return BBGPU_OK;
    }
    // The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and kernels of two streams that
    // share a queue run one after the other.  With the caller's streams beside them the four MSM slot streams landed on TWO queues: "three in
    // flight" was slower than two for that reason alone (rocprofv3 timeline, DESIGN_HISTORY.md 6; 2^16-point MSMs three in flight 0.168 -> 0.127 ms per
    // MSM with 8 queues, a 1/8 share four in flight 0.232 -> 0.205).  16: the eight slot streams, the library's own and the caller's.  Only effective when this is the process's first HIP call; a host
    // program that initialises HIP earlier sets the variable itself (bench.py and the Python binding do).
    (void)setenv("GPU_MAX_HW_QUEUES", "16", 0);
    if (hip_device_count() == 0) {
        set_error("no HIP device available: the GPU entry points of libbbgpu have no CPU fallback");
        return BBGPU_ERR_HIP;
    }
    HIPCHK(hipSetDevice(ctx().device));
    HIPCHK(hipStreamCreateWithFlags(&ctx().stream, hipStreamNonBlocking));
    // the slot streams are made HERE, one after the other: the runtime deals streams to hardware queues in creation order, and a slot
    // stream created later (first use of a third slot, in a process that has made other streams meanwhile) can land on the queue of another slot
    for (auto& sl : ctx().slot) {
        if (!sl.stream) HIPCHK(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
        sl.acc_ring = &ctx().acc_ring;
    }
    HIPCHK(hipEventCreateWithFlags(&ctx().shared_done, hipEventDisableTiming));
    ctx().shared_used = false;
    // the cap holds for each device context on its own (bbgpu_init_devices)
    if (const char* e = getenv("BBGPU_SRS_CACHE_BYTES")) ctx().srs_cache_cap = (size_t)strtoull(e, nullptr, 0);
    if (const char* e = getenv("BBGPU_SRS_VALIDATE")) ctx().srs_validate_full = !strcmp(e, "full"); // full: host-pointer MSMs re-hash every row they use on every call (exact, ~+0.1 ms per 2^16 points hidden behind the kernels); default: 16 sampled rows
    ctx().ready = true;
    return BBGPU_OK;
}

// The NTT scratch and the polynomial temporaries are one set of buffers for all callers.  A call on stream `st` first waits (on the
// device) for the last user if that was another stream, and leaves its own completion event behind: two transforms issued back to
// back on two streams then run one after the other instead of overwriting each other's intermediate data.
int shared_begin(hipStream_t st)
{
    if (ctx().shared_used && ctx().shared_last != st) HIPCHK(hipStreamWaitEvent(st, ctx().shared_done, 0));
    return BBGPU_OK;
}
int shared_end(hipStream_t st)
{
    HIPCHK(hipEventRecord(ctx().shared_done, st));
    ctx().shared_last = st;
    ctx().shared_used = true;
    return BBGPU_OK;
}

int grow(uint64_t** buf, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return BBGPU_OK;
    if (*buf) (void)dev_free(*buf);
    *buf = nullptr;
    *cap = 0;
    HIPCHK(dev_malloc((void**)buf, bytes));
    *cap = bytes;
    return BBGPU_OK;
}

} // namespace

// ---- the callers' host buffers ------------------------------------------------------------------------------------------------------
// A pageable buffer handed to hipMemcpyAsync is pinned in place by the runtime (a userptr mapping it keeps for later copies).  That is
// the fastest path while the caller keeps its buffers -- and a trap when it does not: the reference's Prover allocates its polynomials
// per proof, and when such a pinned range is unmapped the driver quiesces and later restores the process's GPU queues.  Seen from the
// unmodified reference prover linked on the shim (tools/shim_profile.py, BBGPU_TRACE_SRS=1): from the second proof of a process on, one
// hipMemcpyAsync per proof BLOCKED for 6-23 ms (a 2 MiB upload; of a 64 ms proof).  So buffers up to `host_stage_max` (8 MiB: every
// polynomial of a 2^16-gate proof, its 4n-coset vectors and its 8 MiB point table) cross through two pinned 4 MiB buffers of the
// library's own: CPU memcpy (30-50 GB/s on the boxes' EPYC 9575F), DMA from / to pinned memory, the copy of chunk k+1 under the DMA of
// chunk k.  Larger buffers keep the direct path: there a copy is 0.6 ms per 32 MiB against ~1 ms through one staging thread, and the
// stall is small against the work (profiles/r03_pcie.txt).

int bind_calling_thread()
{
    return ensure_init(); // takes the current context's lock
}
static int host_stage_ensure()
{
    for (int k = 0; k < Context::HOST_RING; k++)
        if (!ctx().h_stage[k]) {
            HIPCHK(hipHostMalloc(&ctx().h_stage[k], Context::HOST_CHUNK, hipHostMallocDefault));
            HIPCHK(hipEventCreateWithFlags(&ctx().h_stage_free[k], hipEventDisableTiming));
        }
    return BBGPU_OK;
}
// `bytes` (at most HOST_CHUNK) built by fill(h) in the next pinned buffer of the ring and sent to d_dst in ONE copy; the caller holds the context's lock
template <class Fill> static int stage_head(void* d_dst, size_t bytes, hipStream_t st, Fill fill)
{
    if (int rc = host_stage_ensure()) return rc;
    const int k = (int)(ctx().h_stage_next++ % Context::HOST_RING);
    HIPCHK(hipEventSynchronize(ctx().h_stage_free[k])); // the DMA that last read this buffer has finished (no-op before its first use)
    fill(static_cast<uint8_t*>(ctx().h_stage[k]));
    HIPCHK(h2d_async(d_dst, ctx().h_stage[k], bytes, st));
    HIPCHK(hipEventRecord(ctx().h_stage_free[k], st));
    return BBGPU_OK;
}
// Both directions take the current context's lock themselves -- context 0's is the library mutex (recursive: the capi entry points already hold it):
// the resident prover's uploads (plonk.hip, which holds only its own mutex) would otherwise race with a transform or an MSM of another thread on the
// staging buffers, their events and the single-producer copy pool.  A worker of a split MSM takes its own context's lock (the caller holds g_mu).
// Lock order everywhere: the prover's mutex first, then g_mu, then a worker context's lock.
int host_to_device(void* d_dst, const void* h_src, size_t bytes, hipStream_t st)
{
    std::lock_guard<std::recursive_mutex> lk(ctx_lock());
    read_host_env();
    if (bytes == 0) return BBGPU_OK;
    if (bytes > ctx().host_stage_max) {
        HIPCHK(h2d_async(d_dst, h_src, bytes, st));
        return BBGPU_OK;
    }
    const size_t CH = ctx().host_chunk;
    for (size_t off = 0; off < bytes; off += CH) {
        const size_t len = std::min(CH, bytes - off);
        if (int rc = stage_head((char*)d_dst + off, len, st, [&](uint8_t* h) { ctx().copy_pool.copy(h, (const char*)h_src + off, len); })) return rc;
    }
    return BBGPU_OK;
}
// device -> caller's buffer, complete on return (everything enqueued on `st` before it has run as well).
// *touched (optional): set when the call may have written ANY byte of h_dst -- on a failure that tells an in-place caller whether its input is still
// whole (nothing touched: an ordinary error the shim answers on the host) or gone (BBGPU_ERR_LOST).
int device_to_host_sync(void* h_dst, const void* d_src, size_t bytes, hipStream_t st, bool* touched)
{
    std::lock_guard<std::recursive_mutex> lk(ctx_lock());
    read_host_env();
    if (touched) *touched = false;
    if (bytes > ctx().host_stage_max) {
        HIPCHK(d2h_async(h_dst, d_src, bytes, st));
        if (touched) *touched = true; // the DMA engine owns the destination from here on
        HIPCHK(hipStreamSynchronize(st));
        return BBGPU_OK;
    }
    if (int rc = host_stage_ensure()) return rc;
    // up to HOST_RING - 1 chunks are on the link (or queued for it) while one is copied out of its pinned buffer
    const size_t CH = ctx().host_chunk;
    const size_t chunks = (bytes + CH - 1) / CH;
    constexpr size_t AHEAD = Context::HOST_RING - 1;
    int kbuf[Context::HOST_RING] = {};
    auto enqueue = [&](size_t c) -> int {
        const int k = (int)(ctx().h_stage_next++ % Context::HOST_RING);
        kbuf[c % Context::HOST_RING] = k;
        HIPCHK(hipEventSynchronize(ctx().h_stage_free[k]));
        HIPCHK(d2h_async(ctx().h_stage[k], (const char*)d_src + c * CH, std::min(CH, bytes - c * CH), st));
        HIPCHK(hipEventRecord(ctx().h_stage_free[k], st));
        return BBGPU_OK;
    };
    if (chunks == 0) {
        HIPCHK(hipStreamSynchronize(st));
        return BBGPU_OK;
    }
    size_t queued = 0;
    for (; queued < chunks && queued < AHEAD; queued++)
        if (int rc = enqueue(queued)) return rc;
    for (size_t c = 0; c < chunks; c++) {
        if (queued < chunks) {
            if (int rc = enqueue(queued)) return rc;
            queued++;
        }
        const int k = kbuf[c % Context::HOST_RING];
        HIPCHK(hipEventSynchronize(ctx().h_stage_free[k]));
        if (touched) *touched = true;
        ctx().copy_pool.copy((char*)h_dst + c * CH, ctx().h_stage[k], std::min(CH, bytes - c * CH));
    }
    return BBGPU_OK;
}
void host_stage_release()
{
    std::lock_guard<std::recursive_mutex> lk(ctx_lock());
    ctx().copy_pool.shutdown();
    for (int k = 0; k < Context::HOST_RING; k++) {
        if (ctx().h_stage[k]) (void)hipHostFree(ctx().h_stage[k]);
        if (ctx().h_stage_free[k]) (void)hipEventDestroy(ctx().h_stage_free[k]);
        ctx().h_stage[k] = nullptr;
        ctx().h_stage_free[k] = nullptr;
    }
}

namespace {

constexpr size_t AUTO_REGISTER_MIN_POINTS = 1024; // host-pointer MSMs against unknown tables below this size do not cache the table

// BBGPU_TRACE_SRS=1: one line on stderr per event of the address-keyed point-table cache (register, evict, content mismatch)
bool trace_srs()
{
    static const bool on = getenv("BBGPU_TRACE_SRS") != nullptr;
    return on;
}
void free_entry(SrsEntry& e)
{
    if (trace_srs()) fprintf(stderr, "bbgpu srs: evict %p n=%zu auto=%d\n", (const void*)e.host_ptr, e.n, (int)e.auto_registered);
    // an asynchronous MSM may still be reading the table: drain the device first (rare path)
    (void)hipDeviceSynchronize();
    if (e.d_srs) (void)dev_free(e.d_srs);
    for (auto& sg : e.segs)
        if (sg.d_tab_alloc) (void)dev_free(sg.d_tab_alloc);
    e.segs.clear();
    e.d_srs = nullptr;
    e.live = false;
    e.row_hash.clear();
    e.row_hash.shrink_to_fit();
}
bool ranges_overlap(const SrsEntry& e, const uint64_t* p, size_t n)
{
    const uint8_t *a0 = (const uint8_t*)e.host_ptr, *a1 = a0 + e.n * 128, *b0 = (const uint8_t*)p, *b1 = b0 + n * 128;
    return a0 < b1 && b0 < a1;
}

// registers resident points; builds the pre-shifted window tables when enabled and the 24-bit row index allows it.
// An auto-registered table first evicts the auto-registered tables it overlaps in host memory (they are what used to live there) and
// the least recently used ones beyond the byte cap.
int add_srs(const uint64_t* host_ptr, size_t n, uint32_t* d_srs, bool auto_registered)
{
    if (trace_srs()) fprintf(stderr, "bbgpu srs: register %p n=%zu auto=%d\n", (const void*)host_ptr, n, (int)auto_registered);
    SrsEntry e;
    e.host_ptr = host_ptr;
    e.n = n;
    e.d_srs = d_srs;
    e.live = true;
    e.auto_registered = auto_registered;
    e.validate_full = ctx().srs_validate_full;
    e.last_use = ++ctx().use_clock;
    if (host_ptr) {
        e.row_hash.resize(n);
        struct Job { const uint64_t* p; uint64_t* h; } job{ host_ptr, e.row_hash.data() };
        ctx().copy_pool.for_range(n, (size_t)1 << 14, [](void* c, size_t lo, size_t hi) {
            const Job* j = static_cast<const Job*>(c);
            for (size_t i = lo; i < hi; i++) j->h[i] = hash_row(j->p + i * 16);
        }, &job);
    }
    // a rank's slice of a point-range split takes the window size of the whole MSM: measured on 1/4 and 1/8 slices of 2^20 points, four in flight,
    // 15-bit windows 0.356 / 0.189 ms per step, 17-bit 0.334 / 0.188 (16-bit at 1/8: 0.182) -- tools/slice_ab.py
    // (the slice a context holds of a split host-pointer MSM, bbgpu_init_devices, takes the window size of the whole call in the same way)
    const bool slice = ctx().slice_of_n > n || ctx().point_world > 1;
    const size_t n_for_c = ctx().slice_of_n > n ? ctx().slice_of_n : n * (size_t)ctx().point_world;
    int c = msm_choose_c(n_for_c);
    // with tables every window feeds one shared bucket set, so wider windows only cost bucket-reduction depth while each one
    // saved is n fewer mixed additions: measured on the resident prover (tools/plonk_bench.py), 2^16 gates 3.58 ms at c = 12,
    // 3.40 / 3.54 / 3.36 / 3.40 at c = 13 / 14 / 15 / 16; 2^18 gates 7.51 ms at c = 14, 7.19 at c = 15, 7.20 at c = 16
    if (n_for_c >= ((size_t)1 << 16) && c < 15) c = 15;
    // 17-bit windows (15 instead of 16 of them, signed digits up to +-2^16 kept as uint16 magnitude + sign bit, 2^16 buckets): one n-th fewer mixed additions.
    // Measured: single 2^20 MSM 1.611 -> 1.546 ms, two in flight 1.345 -> 1.287 ms/step (-4.3 %); prover 2^19 gates 11.89 -> 11.51 ms,
    // 2^20 gates 22.1-22.8 -> 22.0 ms; 2^18 gates unchanged (6.8 ms), so smaller tables keep c = 15 (measured again at the end of round 3, tools/plonk_bench.py:
    // 2^17 gates 3.51 / 3.40-3.50 / 3.49-3.52 ms at c = 15 / 16 / 17, 2^18 gates 5.74-5.80 / 5.58-5.87 / 5.58-5.63: within 3 %, and the reference fixtures sit around the 2^19 switch)
    if (n_for_c >= ((size_t)1 << 19)) c = 17;
    // ... but a slice of fewer than 2^18 points pays the row / column sums over 2^16 buckets for ~30 entries per bucket: 16-bit windows (2^15 buckets, one window
    // more) measured 0.179 against 0.182 ms per step at 2^17 points, four in flight, three alternating runs (15-bit windows: 0.189)
    if (slice && c == 17 && n < ((size_t)1 << 18)) c = 16;
    if (const char* ev = getenv("BBGPU_TABLE_C")) c = std::min(17, std::max(4, atoi(ev))); // window size of the tables
    const int W = msm_num_windows(c);
    // segments: as few as the 24-bit row index allows, equal lengths (multiples of 8: the sort reads eight digits per load).  One up to 2^20 points;
    // beyond that the tables are kept up to BBGPU_TABLE_MAX_BYTES (default 64 GiB = 2^26 points) -- larger tables fall back to per-window bucket sets
    static const uint64_t tab_max_bytes = [] { const char* v = getenv("BBGPU_TABLE_MAX_BYTES"); return v ? strtoull(v, nullptr, 0) : (uint64_t)64 << 30; }();
    size_t seg_cap = (size_t)((((uint64_t)1 << 24) / (uint64_t)W) & ~(uint64_t)7);
    // testing knob: smaller segments, so that the piece machinery of the large MSMs can be driven against the oracle at sizes the oracle finishes in seconds
    // (read at registration; the decomposition changes, the sum does not)
    if (const char* v = getenv("BBGPU_TABLE_SEG_POINTS")) seg_cap = std::min(seg_cap, std::max<size_t>(64, (size_t)strtoull(v, nullptr, 0) & ~(size_t)7));
    const size_t nseg = (n + seg_cap - 1) / seg_cap;
    const size_t seg_n = nseg <= 1 ? n : ((((n + nseg - 1) / nseg) + 7) & ~(size_t)7);
    const bool want_tab = ctx().precompute && n >= 1024 && (nseg == 1 || ((uint64_t)n * W * 64 <= tab_max_bytes && nseg <= (size_t)MSM_MAX_PIECES));
    // a rank of an N-way row split touches windows [floor(W r / N), ceil(W (r + 1) / N)) only (bbgpu_set_table_share)
    const int twb = (int)((int64_t)W * ctx().share_rank / ctx().share_world);
    const int twe = (int)(((int64_t)W * (ctx().share_rank + 1) + ctx().share_world - 1) / ctx().share_world);
    e.bytes = n * 64 + (want_tab ? (size_t)(twe - twb) * n * 64 : 0);
    if (auto_registered) {
        for (auto& o : ctx().srs)
            if (o.live && o.auto_registered && o.host_ptr && host_ptr && ranges_overlap(o, host_ptr, n)) free_entry(o);
        for (;;) {
            size_t held = 0;
            SrsEntry* lru = nullptr;
            for (auto& o : ctx().srs)
                if (o.live && o.auto_registered) {
                    held += o.bytes;
                    if (!lru || o.last_use < lru->last_use) lru = &o;
                }
            if (!lru || held + e.bytes <= ctx().srs_cache_cap) break;
            free_entry(*lru);
        }
    }
    if (want_tab) {
        for (size_t first = 0; first < n; first += seg_n) {
            SrsEntry::TabSeg sg;
            sg.first = first;
            sg.n = std::min(seg_n, n - first);
            int rc = srs_build_table(d_srs + first * 16, sg.n, c, W, twb, twe, &sg.d_tab_alloc, &sg.d_tab, ctx().stream);
            if (rc) {
                // no room for the window tables (a shared GPU): the points stay resident and the MSMs over them take one bucket set per window --
                // slower (1.8 ms instead of 1.14 at 2^20) but on the GPU, instead of failing the registration and sending the caller to the host
                for (auto& o : e.segs) (void)dev_free(o.d_tab_alloc);
                e.segs.clear();
                (void)hipGetLastError();
                fault_absorbed();
                fprintf(stderr, "bbgpu: window tables of %zu bytes for an SRS of %zu points could not be built (%s): continuing without them\n",
                        (size_t)(twe - twb) * n * 64, n, g_err);
                g_err[0] = 0;
                break;
            }
            e.segs.push_back(sg);
        }
        if (e.segs.empty()) {
            e.bytes = n * 64;
        } else {
            e.tab_c = c;
            e.tab_W = W;
            e.tab_wb = twb;
            e.tab_we = twe;
        }
    }
    e.handle_exposed = !auto_registered;
    // a long-lived process that keeps re-registering tables on first sight must not grow the registry by one entry per eviction: dead slots
    // whose index no caller ever held are taken again
    if (auto_registered)
        for (size_t k = 0; k < ctx().srs.size(); k++)
            if (!ctx().srs[k].live && !ctx().srs[k].handle_exposed) {
                ctx().srs[k] = std::move(e);
                return (int)k;
            }
    ctx().srs.push_back(std::move(e));
    return (int)ctx().srs.size() - 1;
}
int entry_windows(const SrsEntry& e, size_t n)
{
    return e.has_tab() ? e.tab_W : msm_num_windows(msm_choose_c(n ? n : 1));
}
bool windows_resident(const SrsEntry& e, int wb, int we)
{
    if (!e.has_tab() || (wb >= e.tab_wb && we <= e.tab_we)) return true;
    set_error("windows [%d, %d) requested, this table keeps [%d, %d) of %d (bbgpu_set_table_share)", wb, we, e.tab_wb, e.tab_we, e.tab_W);
    return false;
}
// A free slot for an asynchronous MSM: slots 0 / 1 alternate for consecutive calls (two large MSMs in flight is the measured optimum for the
// full-size pipeline), the others take whatever else is in flight (shares of a split MSM, small MSMs: up to eight).  -1: all busy.
int pick_slot()
{
    int order[Context::NSLOT] = { ctx().next_slot, ctx().next_slot ^ 1 };
    for (int k = 2; k < Context::NSLOT; k++) order[k] = k;
    for (int k = 0; k < Context::NSLOT; k++)
        if (!ctx().slot[order[k]].pending) return order[k];
    set_error("all %d MSM slots are in flight: call bbgpu_msm_g1_wait first", Context::NSLOT);
    return -1;
}
// up to `want` slots that are not in flight, for the synchronous (host-pointer) entry points: they take what is free instead of insisting on
// slots 0 / 1, so a caller that holds asynchronous tickets -- or other threads doing so -- never makes pippenger() fail (the reference calls it
// from inside an OpenMP region, scalar_multiplication.cpp:731-738; calls are serialised by the library mutex, not refused)
int free_slots(int* out, int want)
{
    int got = 0;
    for (int k = 0; k < Context::NSLOT && got < want; k++)
        if (!ctx().slot[k].pending) out[got++] = k;
    return got;
}
// the slots a synchronous entry point cycles its jobs / ranges through: marked for the duration of the call, so that a multi-piece job on one of
// them does not take the other as its helper (it is free NOW and about to carry the next job)
struct SlotReservation {
    int a, b;
    SlotReservation(const int* sl, int n) : a(n > 0 ? sl[0] : -1), b(n > 1 ? sl[1] : -1)
    {
        if (a >= 0) ctx().slot[a].reserved = true;
        if (b >= 0) ctx().slot[b].reserved = true;
    }
    ~SlotReservation()
    {
        if (a >= 0) ctx().slot[a].reserved = false;
        if (b >= 0) ctx().slot[b].reserved = false;
    }
};

// The pieces of the point range [off, off + n) of an entry: one per table segment it touches (one in all without tables or inside one segment).
// -1 (with the error text): more than `cap`.
struct PointPiece {
    const SrsEntry::TabSeg* seg; // null: no tables
    size_t off_in_seg, first, len; // first: offset inside the call's range (and its scalars)
};
int split_pieces(const SrsEntry& e, size_t off, size_t n, PointPiece* out, int cap)
{
    if (!e.has_tab()) {
        out[0] = PointPiece{ nullptr, off, 0, n };
        return 1;
    }
    if (n == 0) { // nothing to add up: any segment will do
        out[0] = PointPiece{ &e.segs[0], 0, 0, 0 };
        return 1;
    }
    int cnt = 0;
    for (const auto& sg : e.segs) {
        const size_t lo = std::max(off, sg.first), hi = std::min(off + n, sg.first + sg.n);
        if (lo >= hi) continue;
        if (cnt == cap) {
            set_error("MSM of %zu points spans more than %d table segments", n, cap);
            return -1;
        }
        out[cnt++] = PointPiece{ &sg, lo - sg.first, lo - off, hi - lo };
    }
    return cnt;
}
constexpr int MAX_POINT_PIECES = MSM_MAX_PIECES;

bool others_pending(const MsmSlot* a, const MsmSlot* b = nullptr)
{
    for (int k = 0; k < Context::NSLOT; k++)
        if (&ctx().slot[k] != a && &ctx().slot[k] != b && ctx().slot[k].pending) return true;
    return false;
}
// collects whatever slot t (and its helper) still has in flight and forgets it: error paths
void drain_ticket(int t)
{
    MsmSlot& S = ctx().slot[t];
    host::Xyzz dump[MSM_MAX_JOBS];
    if (S.helper >= 0) {
        MsmSlot& H = ctx().slot[S.helper];
        if (H.pending) (void)msm_finish_batch(H, dump, nullptr);
        H.is_helper = false;
        S.helper = -1;
    }
    if (S.pending) (void)msm_finish_batch(S, dump, nullptr);
}
// the same for n tickets after a failure: the slots are usable again, and the error text stays the first failure's
void drain_tickets(const int* t, int n)
{
    char keep[sizeof(g_err)];
    memcpy(keep, g_err, sizeof(keep));
    for (int k = 0; k < n; k++) drain_ticket(t[k]);
    memcpy(g_err, keep, sizeof(keep));
}
// Issues `jobs` MSMs (one scalar vector each) over points [off, off + n) of entry e, windows [wb, we), on slot t; `st` = the caller's stream or the
// slot's own.  Inside one table segment (every SRS up to 2^20 points) that is one pass through the kernels.  A range that spans several segments
// is issued as one PIECE per segment, dealt alternately to slot t and -- when one is free -- a HELPER slot with its own stream and workspace, so
// that the digit / sort front of piece k + 1 runs beside the accumulation of piece k exactly as two consecutive MSMs do (DESIGN_HISTORY 5); the helper
// is ordered behind the producer of the scalars by an event when the caller gave a stream.  The ticket stays slot t: finish_ticket() adds up
// both slots' pieces.
int issue_ticket(int t, const SrsEntry& e, size_t off, const uint64_t* const* d_scalars_v, int jobs, size_t n, int wb, int we, hipStream_t st)
{
    MsmSlot& S = ctx().slot[t];
    S.helper = -1;
    S.append = false;
    if (!windows_resident(e, wb, we)) return BBGPU_ERR_STATE;
    PointPiece pc[MAX_POINT_PIECES];
    const int np = split_pieces(e, off, n, pc, MAX_POINT_PIECES);
    if (np < 0) return BBGPU_ERR_SIZE;
    if (np == 1) {
        S.throughput = others_pending(&S);
        const uint32_t* tab = pc[0].seg ? pc[0].seg->d_tab + pc[0].off_in_seg * 16 : nullptr;
        return msm_issue_batch(S, e.d_srs + off * 16, tab, pc[0].seg ? pc[0].seg->n : e.n, e.tab_c, d_scalars_v, jobs, n, wb, we, st, ctx().timing);
    }
    // several pieces: a helper slot for every other one, if any slot is free
    int h = -1;
    {
        int order[Context::NSLOT], cnt = 0;
        if (t < 2) order[cnt++] = t ^ 1; // the pair the two-deep pipeline of large MSMs uses
        for (int k = Context::NSLOT - 1; k >= 2; --k) order[cnt++] = k; // from the top: the low ones are what the next tickets take
        for (int k = 0; k < cnt && h < 0; k++)
            if (order[k] != t && !ctx().slot[order[k]].pending && !ctx().slot[order[k]].reserved) h = order[k];
    }
    MsmSlot* H = h >= 0 ? &ctx().slot[h] : nullptr;
    if (H) {
        // `st` carries the producer of the scalars -- a caller's kernel, or the asynchronous upload host_to_device() queued on the slot's OWN stream
        // (bbgpu_msm_g1 / _batch): the helper's stream starts behind what is enqueued there now, whichever stream that is
        if (!ctx().helper_dep[h]) HIPCHK(hipEventCreateWithFlags(&ctx().helper_dep[h], hipEventDisableTiming));
        HIPCHK(hipEventRecord(ctx().helper_dep[h], st));
        HIPCHK(hipStreamWaitEvent(H->stream, ctx().helper_dep[h], 0));
        H->helper = -1;
    }
    int issued[2] = { 0, 0 };
    int rc = BBGPU_OK;
    // every slot's workspace is sized ONCE, for the largest piece it will carry: (seg / 2, 2 seg + 7) is pieces of seg / 2, seg and seg / 2 + 7 points, and a
    // workspace grown for the second piece would be freed (dev_free waits for the device) under the first one still queued on the stream
    {
        size_t largest[2] = { 0, 0 };
        for (int k = 0; k < np; k++) largest[(H && (k & 1)) ? 1 : 0] = std::max(largest[(H && (k & 1)) ? 1 : 0], pc[k].len);
        for (int side = 0; side < 2 && rc == BBGPU_OK; side++)
            if (largest[side]) rc = (side ? *H : S).ws.ensure(MsmWorkspace::bytes_needed(largest[side], e.tab_c, (we - wb) * jobs, jobs)); // pieces run against window tables: one bucket set per job
        if (rc != BBGPU_OK) return rc;
    }
    for (int k = 0; k < np && rc == BBGPU_OK; k++) {
        const int side = (H && (k & 1)) ? 1 : 0;
        MsmSlot& T = side ? *H : S;
        const uint64_t* sv[MSM_MAX_JOBS];
        for (int j = 0; j < jobs; j++) sv[j] = d_scalars_v[j] + pc[k].first * 4;
        T.append = issued[side] > 0;
        T.throughput = true; // pieces share the chip with each other
        rc = msm_issue_batch(T, e.d_srs + (off + pc[k].first) * 16, pc[k].seg->d_tab + pc[k].off_in_seg * 16, pc[k].seg->n, e.tab_c, sv, jobs, pc[k].len, wb, we,
                             side ? H->stream : st, ctx().timing);
        if (rc == BBGPU_OK) issued[side]++;
    }
    if (H && issued[1] > 0) {
        H->is_helper = true;
        S.helper = h;
    }
    if (rc != BBGPU_OK) drain_tickets(&t, 1);
    return rc;
}
// waits for ticket t and adds up its pieces: one point per job
int finish_ticket(int t, host::Xyzz* results, MsmTiming* timing)
{
    MsmSlot& S = ctx().slot[t];
    const uint32_t jobs = S.jobs;
    const int h = S.helper;
    S.helper = -1;
    int rc = msm_finish_batch(S, results, timing);
    if (h >= 0) {
        MsmSlot& H = ctx().slot[h];
        host::Xyzz more[MSM_MAX_JOBS];
        const int rc2 = msm_finish_batch(H, more, nullptr);
        H.is_helper = false;
        if (rc == BBGPU_OK) rc = rc2;
        if (rc == BBGPU_OK)
            for (uint32_t j = 0; j < jobs; j++) results[j] = host::g1_add(results[j], more[j]);
    }
    return rc;
}

// does the host range [points, points + n) still hold what entry e was uploaded from (rows off .. off + n)?
// 16 rows per check: the first, the last, and 14 evenly spaced ones whose PHASE moves on with every check of this entry, so that a buffer
// rewritten only in the middle (a slice the fixed sample never touched) is caught within a few calls instead of never; the residual window
// (a partial in-place rewrite is served stale until a sampled row falls into it) is stated in include/bbgpu.h.
bool contents_match(SrsEntry& e, size_t off, const uint64_t* points, size_t n)
{
    if (e.row_hash.size() != e.n) return false;
    auto same = [&](size_t i) { return hash_row(points + i * 16) == e.row_hash[off + i]; };
    if (n <= 16) {
        for (size_t i = 0; i < n; i++)
            if (!same(i)) return false;
        return true;
    }
    if (!same(0) || !same(n - 1)) return false;
    const size_t stride = n / 14, phase = (size_t)((e.check_phase++ * 0x9e3779b97f4a7c15ULL) % stride);
    for (size_t k = 0; k < 14; k++)
        if (!same(phase + k * stride)) return false;
    return true;
}

// EXACT mode: every row of the range against the fingerprints taken at upload, spread over the staging pool's threads (64 B read per point:
// 2^16 points ~0.05 ms, 2^20 ~1 ms on the boxes' hosts -- which is why the callers run it AFTER they have issued the call's kernels, beside them)
bool contents_match_full(const SrsEntry& e, size_t off, const uint64_t* points, size_t n)
{
    if (e.row_hash.size() != e.n) return false;
    struct Job { const uint64_t* p; const uint64_t* h; std::atomic<int> bad; } job{ points, e.row_hash.data() + off, { 0 } };
    ctx().copy_pool.for_range(n, (size_t)1 << 14, [](void* c, size_t lo, size_t hi) {
        Job* j = static_cast<Job*>(c);
        uint64_t diff = 0;
        for (size_t i = lo; i < hi; i++) diff |= hash_row(j->p + i * 16) ^ j->h[i];
        if (diff) j->bad.store(1);
    }, &job);
    return job.bad.load() == 0;
}

// The same check in the BACKGROUND (the staging pool's helper threads alone) for a call whose scalars do not cross the link through that pool (uploads above
// host_stage_max go to hipMemcpyAsync as they are): started before the upload, joined when the call's kernels have been issued -- the hash of a 2^20-point table
// (64 MiB of host memory) then runs beside the 32 MiB upload and the launches instead of after them.
struct FullCheckJob {
    const uint64_t* p = nullptr;
    const uint64_t* h = nullptr;
    std::atomic<int> bad{ 0 };
    bool posted = false;
};
void full_check_post(FullCheckJob& job, const SrsEntry& e, size_t off, const uint64_t* points, size_t n)
{
    job.p = points;
    job.h = e.row_hash.data() + off;
    job.bad.store(e.row_hash.size() != e.n ? 1 : 0);
    job.posted = true;
    if (job.bad.load()) return;
    ctx().copy_pool.post_range(n, [](void* c, size_t lo, size_t hi) {
        FullCheckJob* j = static_cast<FullCheckJob*>(c);
        uint64_t diff = 0;
        for (size_t i = lo; i < hi; i++) diff |= hash_row(j->p + i * 16) ^ j->h[i];
        if (diff) j->bad.store(1);
    }, &job);
}
bool full_check_join(FullCheckJob& job) // true: contents match
{
    ctx().copy_pool.join();
    job.posted = false;
    return job.bad.load() == 0;
}

// table lookup by host address, VALIDATED by content: returns entry index and point offset, or -1.  An auto-registered table whose
// address range matches but whose contents do not (the caller freed the table and another landed there, or refilled the buffer) is
// evicted; an explicitly registered one is merely not served (its handle stays valid for the device-pointer entries; in-place mutation
// of a registered table requires bbgpu_srs_release, see bbgpu.h).  Newest entries first.
// deferred_full (optional): set when the entry is in EXACT mode and the caller takes over the full check (contents_match_full, run beside the
// kernels it has issued; a mismatch there = srs_mark_stale + redo); without it the full check runs here.
int find_srs(const uint64_t* points, size_t n, size_t* offset, bool* deferred_full = nullptr)
{
    if (deferred_full) *deferred_full = false;
    for (size_t k = ctx().srs.size(); k-- > 0;) {
        SrsEntry& e = ctx().srs[k];
        if (!e.live || !e.host_ptr || e.stale_for_host) continue;
        const uint8_t* b = (const uint8_t*)e.host_ptr;
        const uint8_t* p = (const uint8_t*)points;
        if (p < b || p >= b + e.n * 128) continue;
        const size_t d = (size_t)(p - b);
        if (d % 128) continue;
        if (d / 128 + n > e.n) continue;
        if (!contents_match(e, d / 128, points, n) || (e.validate_full && !deferred_full && !contents_match_full(e, d / 128, points, n))) {
            if (trace_srs()) fprintf(stderr, "bbgpu srs: contents of %p (+%zu rows, n=%zu) differ from the resident copy\n", (const void*)e.host_ptr, d / 128, n);
            if (e.auto_registered) free_entry(e);
            else if (e.validate_full) e.stale_for_host = true;
            continue;
        }
        if (deferred_full) *deferred_full = e.validate_full;
        e.last_use = ++ctx().use_clock;
        *offset = d / 128;
        return (int)k;
    }
    return -1;
}

// the deferred full check of an exact-mode entry failed: never serve this copy to a host-pointer call again
void srs_mark_stale(int idx)
{
    SrsEntry& e = ctx().srs[idx];
    if (trace_srs()) fprintf(stderr, "bbgpu srs: full check: contents of %p differ from the resident copy\n", (const void*)e.host_ptr);
    if (e.auto_registered) free_entry(e);
    else e.stale_for_host = true;
}

double now_ms() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

// How the host scalars of bbgpu_msm_g1 / _plain / _batch go through the MSM slots: the one place that knows.  A call opens the pipeline on the (up to
// two) slots that are free, PUSHES point ranges against resolved tables -- the ranges of one MSM, or of the jobs of a batch -- and FINISHES.  Ticket k rides
// slot k mod slots with that slot's staging buffer: the scalars of range k+1 cross the link and its kernels are enqueued while the bucket-reduction
// tail and the host finish of range k run (a prover round's 3/1/3/2 MSMs, prover.cpp:65-122,650-658).  Tickets are collected in issue order and their
// sums handed to done(tag, sum).  Whatever fails -- here or in the caller between two pushes -- nothing of the call stays in flight: every slot is
// drained, at once or by the destructor, and the error text stays the first failure's.
size_t largest_piece(const PointPiece* pc, int np) { size_t m = 0; for (int k = 0; k < np; k++) m = std::max(m, pc[k].len); return m; }
// tickets of a pipeline on `slots` slots that have been collected once room is made for push number p: all but the slots - 1 before it
size_t collected_before(size_t p, int slots) { return p - std::min(p, (size_t)std::max(slots, 1) - 1); }
template <class Done> struct HostMsmPipeline { // Done: void(size_t tag, const host::Xyzz& sum)
    int sl[2] = { -1, -1 }, ns = 0; // whatever slots are free (a caller -- or another thread -- may hold asynchronous tickets on any of them): two give the pipeline, one works
    Done done;
    double ms_push = 0, ms_wait = 0; // BBGPU_TRACE_SRS: time spent so far in uploads + launches, in collections

    explicit HostMsmPipeline(Done d) : done(std::move(d)) {}
    HostMsmPipeline(const HostMsmPipeline&) = delete;
    ~HostMsmPipeline()
    {
        if (bg.posted) (void)full_check_join(bg); // the job reads the caller's table and the entry's fingerprints
        drain();
    }
    int open()
    {
        if (int rc = ensure_init()) return rc;
        if ((ns = free_slots(sl, 2)) == 0) {
            set_error("all %d MSM slots are in flight: call bbgpu_msm_g1_wait first", Context::NSLOT);
            return BBGPU_ERR_STATE;
        }
        reserve.emplace(sl, ns); // the slots of the rotation are nobody's helper (every push lies inside one table segment and asks for none itself)
        return BBGPU_OK;
    }
    hipStream_t first_stream() const { return ctx().slot[sl[0]].stream; } // of the slot the first push takes
    // frees the slot and staging buffer of the next push: collects the ticket that still holds them
    int make_room() { return collected < collected_before(issued, ns) ? collect() : BBGPU_OK; }
    // host scalars [0, len) against points [off, off + len) of e; stage_bytes: the largest range the caller will push (the staging buffers are sized once)
    int push(const SrsEntry& e, size_t off, const uint64_t* scalars, size_t len, size_t stage_bytes, size_t tag, MsmTiming* timing)
    {
        if (int rc = make_room()) return rc;
        const size_t w = issued % (size_t)ns;
        MsmSlot& S = ctx().slot[sl[w]];
        const double t0 = tr ? now_ms() : 0;
        int rc = grow(stage[w], cap[w], stage_bytes);
        if (rc == BBGPU_OK) rc = host_to_device(*stage[w], scalars, len * 32, S.stream);
        if (rc == BBGPU_OK) rc = issue_ticket(sl[w], e, off, stage[w], 1, len, 0, entry_windows(e, len), S.stream);
        if (rc) { drain(); return rc; }
        if (tr) ms_push += now_ms() - t0;
        fl[w] = InFlight{ tag, timing };
        issued++;
        return BBGPU_OK;
    }
    // EXACT mode: rows [off, off + n) of entry idx are compared in full with the caller's table by finish(), once per distinct range, on the host beside
    // the kernels issued by then.  background: the call's scalars bypass the staging pool (uploads above host_stage_max go to hipMemcpyAsync as they
    // are), so the check starts NOW on the pool's helper threads -- before the upload -- and is joined in finish()
    void check_in_full(int idx, size_t off, const uint64_t* points, size_t n, bool background)
    {
        for (const auto& c : checks)
            if (c.idx == idx && c.off == off && c.n == n) return;
        if (background && checks.empty()) full_check_post(bg, ctx().srs[idx], off, points, n);
        checks.push_back(Check{ idx, off, points, n });
    }
    // the exact-mode checks, then the collection of what is in flight.  *stale: a resident table differs from the caller's memory and was dropped;
    // nothing is in flight, and what done() has been handed came from the stale copy: the caller's rerun replaces all of it
    int finish(bool* stale)
    {
        for (size_t k = 0; k < checks.size(); k++) {
            const Check& c = checks[k];
            const bool same = (k == 0 && bg.posted) ? full_check_join(bg) : !ctx().srs[c.idx].live || contents_match_full(ctx().srs[c.idx], c.off, c.points, c.n);
            if (!same) {
                srs_mark_stale(c.idx);
                *stale = true;
            }
        }
        if (*stale) {
            drain();
            return BBGPU_OK;
        }
        while (collected < issued)
            if (int rc = collect()) return rc;
        return BBGPU_OK;
    }

private:
    struct InFlight { size_t tag; MsmTiming* timing; } fl[2] = {};
    size_t issued = 0, collected = 0;
    uint64_t** stage[2] = { &ctx().d_stage, &ctx().d_stage2 };
    size_t* cap[2] = { &ctx().stage_cap, &ctx().stage2_cap };
    std::optional<SlotReservation> reserve;
    struct Check { int idx; size_t off; const uint64_t* points; size_t n; };
    std::vector<Check> checks;
    FullCheckJob bg; // checks[0], when it runs in the background
    const bool tr = trace_srs();

    int collect() // the oldest ticket in flight
    {
        const size_t w = collected++ % (size_t)ns;
        const double t0 = tr ? now_ms() : 0;
        host::Xyzz sum;
        if (int rc = finish_ticket(sl[w], &sum, fl[w].timing)) { drain(); return rc; }
        done(fl[w].tag, sum);
        if (tr) ms_wait += now_ms() - t0;
        return BBGPU_OK;
    }
    void drain() // nothing of the call stays in flight
    {
        drain_tickets(sl, ns);
        collected = issued;
    }
};

// EXACT cache mode: a call runs against the resident copy of a table while the host re-hashes every row of the caller's; if they differ the copy is
// dropped and the call runs once more, now uploading the table as it is (the reference reads the caller's points on every call,
// scalar_multiplication.cpp:604-617).  Exactly one rerun.
template <class Once> int rerun_if_stale(Once once)
{
    bool stale = false;
    int rc = once(&stale);
    if (stale) rc = once(&stale);
    return rc;
}

int log2_exact(size_t n)
{
    if (n == 0 || (n & (n - 1))) return -1;
    int l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}

// plain: `points` is an n-entry table of plain affine points (64 bytes apart) instead of the 2n-entry endomorphism table -- the argument of
// the reference's pippenger_low_memory / pippenger_precomputed (scalar_multiplication.cpp:142-262, :478-574).  Such a table is used once and
// forgotten (no address-keyed cache: these are test / bench entries of the reference, not the prover's).
int msm_host_ptrs_once(const uint64_t* scalars, const uint64_t* points, size_t n, host::Xyzz* out, bool plain, bool* stale);
// the sum before normalisation: a context's partial sum of a split call (bbgpu_msm_g1) is added to the others' first
int msm_host_ptrs_sum(const uint64_t* scalars, const uint64_t* points, size_t n, host::Xyzz* out, bool plain = false)
{
    return rerun_if_stale([&](bool* stale) { return msm_host_ptrs_once(scalars, points, n, out, plain, stale); });
}
int msm_host_ptrs(const uint64_t* scalars, const uint64_t* points, size_t n, uint64_t out[12], bool plain = false)
{
    host::Xyzz res;
    const int rc = msm_host_ptrs_sum(scalars, points, n, &res, plain);
    if (rc == BBGPU_OK) host::g1_to_normalised(res, out);
    return rc;
}
int msm_host_ptrs_once(const uint64_t* scalars, const uint64_t* points, size_t n, host::Xyzz* out, bool plain, bool* stale)
{
    *stale = false;
    if (n == 0) {
        *out = host::g1_infinity();
        return BBGPU_OK;
    }
    if (!scalars || !points) {
        set_error("null scalars/points");
        return BBGPU_ERR_ARG;
    }
    size_t off = 0;
    bool full_check = false;
    int idx = plain ? -1 : find_srs(points, n, &off, &full_check);
    read_host_env();
    if (idx < 0 && n <= (size_t)ctx().host_msm_max) { // the verifier's ~20 freshly built points: no allocation, no launch
        *out = host::msm_small(scalars, points, n, plain ? 8 : 16);
        return BBGPU_OK;
    }
    host::Xyzz res = host::g1_infinity();
    HostMsmPipeline P([&res](size_t, const host::Xyzz& part) { res = host::g1_add(res, part); });
    if (int rc = P.open()) return rc;
    // exact cache mode on a table large enough that the scalars bypass the staging pool: the full check starts NOW, before the upload
    if (full_check) P.check_in_full(idx, off, points, n, n * 32 > ctx().host_stage_max);
    // A table that was never registered and is too small to be an SRS (the verifier's ~20 freshly built points,
    // verifier.cpp:359-363) is used once and forgotten: caching it by address would both leak device memory per call and
    // serve stale points when the caller's vector is freed and its address reused.  Larger unknown tables are taken to be a
    // long-lived SRS and registered on first sight.
    SrsEntry transient{};
    const bool is_transient = idx < 0 && (plain || n < AUTO_REGISTER_MIN_POINTS);
    const bool tr = trace_srs();
    const double q0 = tr ? now_ms() : 0;
    // a small table that is used once (the verifier's freshly built points, test tables): uploaded into a buffer the library keeps, on the stream of the
    // slot that runs the call's one range -- no allocation, no free, no wait (round 5: those were ~0.05 of the 0.39 ms such a call took)
    const bool small_once = is_transient && n < AUTO_REGISTER_MIN_POINTS;
    if (idx < 0) {
        uint32_t* d = nullptr;
        int rc = BBGPU_OK;
        if (small_once) {
            if ((rc = grow(&ctx().d_small_tab, &ctx().small_tab_cap, AUTO_REGISTER_MIN_POINTS * (128 + 64))) != BBGPU_OK) return rc;
            uint32_t* d_raw = (uint32_t*)ctx().d_small_tab;
            d = d_raw + AUTO_REGISTER_MIN_POINTS * 32;
            rc = srs_upload_into(points, n, d_raw, d, P.first_stream(), plain ? 64 : 128);
        } else {
            rc = srs_upload(points, n, &d, ctx().stream, plain ? 64 : 128);
        }
        if (rc) return rc;
        if (is_transient) {
            transient.host_ptr = points;
            transient.n = n;
            transient.d_srs = d;
            transient.live = true;
        } else if ((idx = add_srs(points, n, d, true)) < 0) {
            return idx;
        }
        off = 0;
    }
    const SrsEntry& e = is_transient ? transient : ctx().srs[idx];
    // The call is cut into point RANGES that go through the free slots like the jobs of a batch: the scalars of range k+1 cross the link while
    // the kernels of range k run, and the partial sums (group elements: the sum over a range of points is a plain term of the whole sum) are
    // added on the host.  Above 2^20 points the ranges are the table segments the call touches (each at most 2^20 points with its own window
    // tables); inside one segment a call of 2^19 points and more is cut in two -- one 2^20-point call: 32 MiB of scalars = 0.6 ms on the link
    // before the first kernel, against 0.22 ms for the first of two ranges (bench.py `boundary`).  BBGPU_HOST_MSM_SPLIT=1 keeps one range per segment.
    static const size_t split_env = [] { const char* v = getenv("BBGPU_HOST_MSM_SPLIT"); return v ? (size_t)std::min(MAX_POINT_PIECES, std::max(1, atoi(v))) : (size_t)0; }();
    PointPiece pc[MAX_POINT_PIECES]; // the ranges: .first and .len are what the loop below reads
    int np = split_pieces(e, off, n, pc, MAX_POINT_PIECES);
    if (np < 0) return BBGPU_ERR_SIZE; // (not a transient table: those have no segments)
    if (np == 1) {
        // Measured on MI355X (tools/boundary_ab.py, 2^20 points): one range 2.05-2.08 ms, two 1.77 ms, four 2.17-2.20 ms -- every range pays its
        // own sort and bucket-reduction tail (~0.3 ms of launches that only partly hide), so two it is, the first one the smaller: its
        // upload is the part nothing hides, and the second range's upload (0.6 ms x its share) still fits under the first one's kernels.
        const size_t parts = P.ns < 2 ? 1 : (split_env ? split_env : (n >= ((size_t)1 << 19) ? 2 : 1));
        // first range 3/8 of the points; measured 25 / 30 / 34 / 37 / 42 %: 1.84 / 1.80 / 1.83 / 1.775 / 1.79 ms
        const size_t base = parts == 2 ? ((n * 3 / 8) & ~(size_t)7) : n / parts;
        np = 0;
        for (size_t k = 0; k < parts; k++) {
            const size_t o = k * base, len = (k + 1 == parts) ? n - o : base;
            if (len) pc[np++] = PointPiece{ nullptr, 0, o, len };
        }
    }
    const size_t stage_bytes = largest_piece(pc, np) * 32;
    const double q1 = tr ? now_ms() : 0;
    int rc = BBGPU_OK;
    for (int k = 0; k < np && rc == BBGPU_OK; k++)
        rc = P.push(e, off + pc[k].first, scalars + pc[k].first * 4, pc[k].len, stage_bytes, (size_t)k, k + 1 == np ? &ctx().last : nullptr);
    if (rc == BBGPU_OK) rc = P.finish(stale);
    const double q3 = tr ? now_ms() : 0;
    if (is_transient && !small_once) (void)dev_free(transient.d_srs); // the pipeline has waited for the kernels
    if (rc || *stale) return rc;
    *out = res;
    if (tr) fprintf(stderr, "bbgpu msm n=%zu: table %.3f, upload + issue %.3f, wait + host sums %.3f, free %.3f ms\n", n, q1 - q0, P.ms_push, P.ms_wait, now_ms() - q3);
    return BBGPU_OK;
}

// ---- device contexts of bbgpu_init_devices ----------------------------------------------------------------------------------------------
// The persistent thread of context k >= 1: created by bbgpu_init_devices, joined by bbgpu_shutdown, one job at a time with context k current.  Its
// first job binds it (ensure_init: hipSetDevice once, then streams and slots on that device).  Allocated and never destroyed at process exit: a
// process that ends without bbgpu_shutdown() leaves the thread waiting instead of destroying a joinable std::thread.
struct MultiWorker {
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    bool busy = false, stop = false;
    int rc = BBGPU_OK;
    std::exception_ptr ex; // what the job threw, handed to the caller (who rethrows it once every context has returned)
    char err[sizeof(g_err)] = "";
    std::thread th; // started in the constructor's body: every member above exists before the thread can touch it
    explicit MultiWorker(int k) { th = std::thread([this, k] { loop(k); }); }
    void loop(int k)
    {
        t_ctx = k;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return stop || job; });
            if (!job) return; // stop, nothing posted
            std::function<int()> fn = std::move(job);
            job = nullptr;
            lk.unlock();
            g_err[0] = 0;
            int r = BBGPU_ERR_STATE;
            std::exception_ptr e;
            try {
                r = fn();
            } catch (...) {
                e = std::current_exception();
            }
            lk.lock();
            rc = r;
            ex = e;
            memcpy(err, g_err, sizeof(err));
            busy = false;
            cv.notify_all();
        }
    }
    void post(std::function<int()> fn)
    {
        std::lock_guard<std::mutex> lk(mu);
        job = std::move(fn);
        busy = true;
        cv.notify_all();
    }
    int wait(char* err_out, std::exception_ptr* ex_out = nullptr) // the job's return code; its error text to err_out, what it threw to *ex_out
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !busy; });
        memcpy(err_out, err, sizeof(err));
        if (ex_out) *ex_out = ex;
        ex = nullptr;
        return rc;
    }
    void join()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            cv.notify_all();
        }
        th.join();
    }
};
MultiWorker* g_workers[BBGPU_MAX_CONTEXTS] = {}; // [0] stays null: context 0 runs on the calling thread

// Runs fn(k) for every k < m at once: k = 0 on the calling thread (which holds g_mu, context 0's lock), k >= 1 on context k's worker.  Returns when
// all have returned -- each context drains its own slots on a failure, so nothing of the call is still in flight -- with the first failure in context
// order as the caller's error, named by context and device.
// An exception (a host allocation, say) is not caught for the caller: the first one in context order is rethrown, but only after every worker has
// returned, since the workers use `fn` and what it refers to on the caller's stack.
int run_on_contexts(int m, const std::function<int(int)>& fn)
{
    for (int k = 1; k < m; k++) g_workers[k]->post([&fn, k] { return fn(k); });
    std::exception_ptr thrown;
    int rc = BBGPU_ERR_STATE;
    try {
        rc = fn(0);
    } catch (...) {
        thrown = std::current_exception();
    }
    int bad = rc ? 0 : -1;
    char text[sizeof(g_err)];
    memcpy(text, g_err, sizeof(text));
    for (int k = 1; k < m; k++) {
        char e[sizeof(g_err)];
        std::exception_ptr ex;
        const int r = g_workers[k]->wait(e, &ex);
        if (ex && !thrown) thrown = ex;
        if (r != BBGPU_OK && bad < 0) {
            rc = r;
            bad = k;
            memcpy(text, e, sizeof(text));
        }
    }
    if (thrown) std::rethrow_exception(thrown);
    if (bad >= 0) {
        text[sizeof(text) - 1] = 0;
        set_error("context %d (device %d): %s", bad, g_ctxs[bad].device, text);
    }
    return rc;
}

// ---- opening sessions (bbgpu_lagrange_opening_*, below): the inverses 1 / (z_t - w^i) of up to BBGPU_OPENING_MAX_POINTS points on one domain, made once by
// begin and kept in an allocation of the session's own until end or bbgpu_shutdown.  Context 0, under g_mu.
struct OpeningSession {
    bool live = false;
    int log2n = 0, points = 0;
    host::Fr z[BBGPU_OPENING_MAX_POINTS]; // canonical
    bool on[BBGPU_OPENING_MAX_POINTS];    // z_t = w^(m_t): the host's verdict, taken once
    size_t m[BBGPU_OPENING_MAX_POINTS];
    uint64_t* d_inv = nullptr;            // points x n elements, point-major
    size_t bytes = 0;
};
OpeningSession g_opening[BBGPU_OPENING_MAX_SESSIONS];
size_t opening_session_bytes()
{
    size_t b = 0;
    for (const auto& o : g_opening)
        if (o.live) b += o.bytes;
    return b;
}
void opening_release(OpeningSession& o)
{
    if (o.live && o.d_inv) (void)dev_free(o.d_inv);
    o = OpeningSession();
}

// ---- setups of bbgpu_kzg_open_all_* and bbgpu_kzg_open_cosets_* (below): S^(e) = DFT_M(s^(e)), e < l, of one (string, n, l, d), d the degree bound (n
// without one): l x M = 2 d scratch points made once by the setup entry and kept in an allocation of the setup's own until its release or bbgpu_shutdown.
// An open-all setup is l = 1, d = n.  Each family has a pool of its own: a handle of one is nothing to the other.  Context 0, under g_mu.
struct OpenSetup {
    bool live = false;
    int log2n = 0, log2l = 0, log2d = 0;
    uint32_t* d_S = nullptr;
    size_t bytes = 0;
};
constexpr int OPEN_MAX_SETUPS = 16;
static_assert(BBGPU_KZG_OPEN_ALL_MAX_SETUPS == OPEN_MAX_SETUPS && BBGPU_KZG_OPEN_COSETS_MAX_SETUPS == OPEN_MAX_SETUPS, "the two pools of open setups: 16 each");
using OpenPool = OpenSetup[OPEN_MAX_SETUPS];
OpenPool g_open_all, g_open_cosets;
size_t open_setup_bytes(const OpenPool& pool)
{
    size_t b = 0;
    for (const auto& o : pool)
        if (o.live) b += o.bytes;
    return b;
}
void open_release(OpenSetup& o)
{
    if (o.live && o.d_S) (void)dev_free(o.d_S);
    o = OpenSetup();
}

// Everything the current context holds, on the thread that drives it (its device is that thread's current one).  Context 0 (primary) also owns the
// resident prover and the transforms' tables.
void release_context(bool primary)
{
    Context& C = ctx();
    if (!C.ready) return;
    if (primary) plonk_release_all_locked();
    if (primary)
        for (auto& o : g_opening) opening_release(o);
    if (primary)
        for (auto& o : g_open_all) open_release(o);
    if (primary)
        for (auto& o : g_open_cosets) open_release(o);
    // nothing may still be reading the pinned staging buffers or a slot's workspace when they are freed: collect what is in flight
    // (an MSM a caller never waited for, a copy queued before an error return) and drain every stream first
    for (int k = 0; k < Context::NSLOT; k++)
        if (C.slot[k].pending && !C.slot[k].is_helper) drain_ticket(k);
    for (auto& ev : C.helper_dep) {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    (void)hipStreamSynchronize(C.stream);
    for (auto& sl : C.slot)
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    (void)hipDeviceSynchronize();
    host_stage_release();
    C.poly_scratch.release();
    if (C.d_poly_tmp) (void)dev_free(C.d_poly_tmp);
    C.d_poly_tmp = nullptr;
    C.poly_tmp_cap = 0;
    for (auto& e : C.srs) {
        if (e.live && e.d_srs) (void)dev_free(e.d_srs);
        if (e.live)
            for (auto& sg : e.segs)
                if (sg.d_tab_alloc) (void)dev_free(sg.d_tab_alloc);
    }
    C.srs.clear();
    for (auto& sl : C.slot) sl.release();
    C.acc_ring.release();
    if (C.d_stage) (void)dev_free(C.d_stage);
    if (C.d_stage2) (void)dev_free(C.d_stage2);
    C.d_stage2 = nullptr;
    C.stage2_cap = 0;
    if (C.d_scratch) (void)dev_free(C.d_scratch);
    C.d_stage = C.d_scratch = nullptr;
    C.stage_cap = C.scratch_cap = 0;
    if (C.d_small_tab) (void)dev_free(C.d_small_tab);
    C.d_small_tab = nullptr;
    C.small_tab_cap = 0;
    if (C.d_srs_check) (void)dev_free(C.d_srs_check);
    C.d_srs_check = nullptr;
    C.srs_check_cap = 0;
    if (C.d_verify) (void)dev_free(C.d_verify);
    C.d_verify = nullptr;
    C.verify_cap = 0;
    if (C.d_kzg_check) (void)dev_free(C.d_kzg_check);
    C.d_kzg_check = nullptr;
    C.kzg_check_cap = 0;
    if (primary) ntt_release_tables();
    if (C.shared_done) (void)hipEventDestroy(C.shared_done);
    C.shared_done = nullptr;
    C.shared_used = false;
    (void)hipStreamDestroy(C.stream);
    C.stream = nullptr;
    C.ready = false;
}

// caller holds the prover's mutex and g_mu
void shutdown_locked()
{
    for (int k = g_num_ctx - 1; k >= 1; k--) {
        if (!g_workers[k]) continue;
        char e[sizeof(g_err)];
        g_workers[k]->post([] { release_context(false); return BBGPU_OK; });
        (void)g_workers[k]->wait(e);
        g_workers[k]->join();
        delete g_workers[k];
        g_workers[k] = nullptr;
    }
    g_num_ctx = 1;
    release_context(true);
}

// one context's share of bbgpu_memory_stats, added to *out
void add_context_memory(const Context& C, bool primary, bbgpu_memory_info* out)
{
    for (const auto& e : C.srs) {
        if (!e.live) continue;
        const uint64_t pts = (uint64_t)e.n * 64, tab = e.bytes > pts ? e.bytes - pts : 0;
        out->srs_points_bytes += pts;
        out->srs_table_bytes += tab;
        if (e.auto_registered) out->srs_auto_bytes += e.bytes;
    }
    out->srs_cache_cap_bytes += C.srs_cache_cap;
    if (primary) {
        size_t cap = 0;
        int sets = 0;
        out->ntt_table_bytes += ntt_table_bytes(&cap, &sets);
        out->ntt_table_cap_bytes += cap;
        out->ntt_table_sets += (uint64_t)sets;
    }
    for (const auto& sl : C.slot) {
        out->msm_workspace_bytes += sl.ws.cap;
        if (sl.ws.h_out) out->pinned_host_bytes += (uint64_t)MSM_HOUT_GROUPS * 64 * 128;
    }
    out->staging_bytes += C.stage_cap + C.stage2_cap + C.scratch_cap + C.poly_tmp_cap + C.poly_scratch.cap + C.small_tab_cap + C.srs_check_cap + C.verify_cap + C.kzg_check_cap;
    if (primary) out->staging_bytes += plonk_lane_bytes() + opening_session_bytes() + open_setup_bytes(g_open_all) + open_setup_bytes(g_open_cosets); // the resident prover, the opening sessions and the open-all and open-cosets setups live on context 0
    for (int k = 0; k < Context::HOST_RING; k++)
        if (C.h_stage[k]) out->pinned_host_bytes += Context::HOST_CHUNK;
}

// ---- what the asynchronous MSM entries and the pairing checks' drivers share ------------------------------------------------------------------------
// srs_live: the handle names a live table.  ticket_srs: the library is up, and that.  begin_ticket: a free slot (slots 0 and 1
// alternate -- the two-deep pipeline of consecutive large MSMs: measured 1.50 ms/step against 1.72 when four streams rotate, more streams than
// hardware queues delay the next MSM's sort behind the previous one's tail -- and the others only take the overflow when both are busy, a prover
// round's three side-by-side commitments), the caller's stream or the slot's own, and the slot's issue flags as a single-piece MSM wants them
// (issue_ticket sets its own).  commit_ticket: the issue went through, the ticket is the slot.
int srs_live(int srs_handle, const SrsEntry** e)
{
    if (srs_handle < 0 || srs_handle >= (int)ctx().srs.size() || !ctx().srs[srs_handle].live) {
        set_error("unknown SRS handle %d", srs_handle);
        return BBGPU_ERR_ARG;
    }
    *e = &ctx().srs[srs_handle];
    return BBGPU_OK;
}
int ticket_srs(int srs_handle, const SrsEntry** e)
{
    if (int rc = ensure_init()) return rc;
    return srs_live(srs_handle, e);
}
// a live table of at least n rows, for the entries that read rows [0, n) of a handle: an argument error, before a device is bound (a handle can only exist
// once one is).  what: the operation, for the text; too_many_code: what n above the table's size is to this entry
int srs_rows(const char* what, int srs_handle, size_t n, int too_many_code, const SrsEntry** e, bool name_handle = false)
{
    if (int rc = srs_live(srs_handle, e)) return rc;
    if (n <= (*e)->n) return BBGPU_OK;
    if (name_handle) set_error("%s of %zu rows, the table of handle %d holds %zu", what, n, srs_handle, (*e)->n);
    else set_error("%s of %zu rows, the table holds %zu", what, n, (*e)->n);
    return too_many_code;
}
int begin_ticket(void* hip_stream, int* t, hipStream_t* st)
{
    if ((*t = pick_slot()) < 0) return BBGPU_ERR_STATE;
    MsmSlot& S = ctx().slot[*t];
    *st = hip_stream ? (hipStream_t)hip_stream : S.stream;
    S.helper = -1;
    S.append = false;
    S.throughput = others_pending(&S);
    return BBGPU_OK;
}
int commit_ticket(int t)
{
    if (t < 2) ctx().next_slot = t ^ 1;
    return t;
}

// A and B of a random-combination check: two tickets in flight, ma scalars at d_a against rows [off_a, off_a + ma) of ea and the same for B, every window of
// each table.  On a failure none is outstanding.
int two_msms(const SrsEntry& ea, size_t off_a, const uint64_t* d_a, size_t ma, const SrsEntry& eb, size_t off_b, const uint64_t* d_b, size_t mb, uint64_t* a12,
             uint64_t* b12)
{
    int ta, tb;
    hipStream_t sa, sb;
    if (int rc = begin_ticket(nullptr, &ta, &sa)) return rc;
    if (int rc = issue_ticket(ta, ea, off_a, &d_a, 1, ma, 0, entry_windows(ea, ma), sa)) return rc;
    commit_ticket(ta);
    int rc = begin_ticket(nullptr, &tb, &sb);
    if (rc == BBGPU_OK && (rc = issue_ticket(tb, eb, off_b, &d_b, 1, mb, 0, entry_windows(eb, mb), sb)) == BBGPU_OK) commit_ticket(tb);
    if (rc != BBGPU_OK) {
        drain_tickets(&ta, 1);
        return rc;
    }
    if (int rcw = bbgpu_msm_g1_wait(ta, a12)) {
        drain_tickets(&tb, 1);
        return rcw;
    }
    return bbgpu_msm_g1_wait(tb, b12);
}
// rows a kernel of the call wrote, as a transient table for two_msms: no window tables
SrsEntry transient_table(uint32_t* d_rows, size_t n)
{
    SrsEntry e{};
    e.n = n;
    e.d_srs = d_rows;
    e.live = true;
    return e;
}

// the call's seed: the caller's, or drawn from the operating system
int call_seed(const char* what, const uint64_t* seed, uint64_t sd[4])
{
    if (host::srs_check_seed(seed, sd)) return BBGPU_OK;
    set_error("%s: the operating system gave no randomness", what);
    return BBGPU_ERR_STATE;
}

// an affine point in memory form (Montgomery-256, any representative) as a resident row: Montgomery-261 (x 2^5), canonical
void resident_row(const uint64_t p[8], uint64_t out[8])
{
    host::Fq v[2];
    host::g1_words_canonical(p, &v[0], &v[1]);
    for (host::Fq& c : v)
        for (int i = 0; i < 5; i++) c = host::fq_dbl(c);
    memcpy(out, v, 64);
}

// The curve pass of bbgpu_srs_check over rows [0, n) of a resident table, for every entry that reads one: the shared staging grown to its 64-byte head (the
// findings, padded: what lies behind them stays 16-byte aligned) and `extra` bytes, `records` (1 or 2) findings started by ONE upload -- the second is for a
// later kernel of the caller's, at findings + 1 --, the kernel, beside(d_extra, st) -- whatever else the caller wants on the stream before the read-back --
// and ONE synchronisation.  generator_m261: the row first_is_generator compares row 0 with (null: the verdict is not used).
const SrsCurveFindings NO_FINDINGS = { 0, ~0ull, 0, 0 };
template <class Beside>
int curve_pass(const uint32_t* d_rows, size_t n, const uint64_t* generator_m261, size_t extra, int records, Beside beside, uint64_t* bad_points,
               uint64_t* first_bad_point, uint32_t* first_is_generator = nullptr)
{
    static_assert(2 * sizeof(SrsCurveFindings) <= 64, "two findings fit the head of the staging");
    if (int rc = grow(&ctx().d_srs_check, &ctx().srs_check_cap, 64 + extra)) return rc;
    SrsCurveFindings* d_find = reinterpret_cast<SrsCurveFindings*>(ctx().d_srs_check);
    const hipStream_t st = ctx().stream;
    const uint64_t no_generator[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    const SrsCurveFindings init[2] = { NO_FINDINGS, NO_FINDINGS };
    SrsCurveFindings got = NO_FINDINGS;
    HIPCHK(h2d_async(d_find, init, (size_t)records * sizeof init[0], st));
    if (int rc = srs_check_curve(d_rows, n, generator_m261 ? generator_m261 : no_generator, d_find, st)) return rc;
    if (int rc = beside(ctx().d_srs_check + 8, st)) return rc;
    HIPCHK(d2h_async(&got, d_find, sizeof got, st));
    HIPCHK(hipStreamSynchronize(st));
    *bad_points = got.bad_points;
    *first_bad_point = got.bad_points ? got.first_bad_point : UINT64_MAX;
    if (first_is_generator) *first_is_generator = got.first_is_generator;
    return BBGPU_OK;
}
int curve_pass(const uint32_t* d_rows, size_t n, int records, uint64_t* bad_points, uint64_t* first_bad_point)
{
    return curve_pass(d_rows, n, nullptr, 0, records, [](uint64_t*, hipStream_t) { return (int)BBGPU_OK; }, bad_points, first_bad_point);
}

// bbgpu_plonk_verify_last_timing, bbgpu_kzg_check_last_timing: wall ms of the last call between the synchronisations it makes anyway -- [0] the call, [1] up to
// the first synchronisation, [2] the folds, [3] the MSMs, [4] the rest: the pairing checks (and the normalisations around them)
struct StageClock {
    double ms[5] = { 0, 0, 0, 0, 0 }, t_begin = 0;
    void begin()
    {
        for (double& v : ms) v = 0;
        t_begin = now_ms();
    }
    void first_sync() { ms[1] = now_ms() - t_begin; }
    void end()
    {
        ms[0] = now_ms() - t_begin;
        ms[4] = ms[0] - ms[1] - ms[2] - ms[3];
    }
    int read(double ms_out[5]) const
    {
        if (!ms_out) return BBGPU_ERR_ARG;
        for (int i = 0; i < 5; i++) ms_out[i] = ms[i];
        return BBGPU_OK;
    }
};
StageClock g_verify_clock, g_kzg_check_clock;

} // namespace
} // namespace bbgpu

using namespace bbgpu;

#pragma GCC visibility push(default)
extern "C" {

const char* bbgpu_version(void) { return "bbgpu 0.1 (gfx950)"; }
const char* bbgpu_last_error(void) { return g_err; }

int bbgpu_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

int bbgpu_init(int device)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (ctx().ready && ctx().device == device) return BBGPU_OK;
    if (ctx().ready) {
        set_error("already bound to %d context(s), the first on device %d: bbgpu_shutdown() first", g_num_ctx, ctx().device);
        return BBGPU_ERR_STATE;
    }
    ctx().device = device;
    return ensure_init();
}

int bbgpu_init_devices(const int* devices, int count)
{
    // argument checks before any HIP call: they hold on a machine without a GPU as well
    if (!devices || count < 1 || count > BBGPU_MAX_CONTEXTS) {
        set_error("bbgpu_init_devices: %s (1 to %d contexts)", devices ? "bad context count" : "null device list", BBGPU_MAX_CONTEXTS);
        return BBGPU_ERR_ARG;
    }
    for (int k = 0; k < count; k++)
        if (devices[k] < 0) {
            set_error("bbgpu_init_devices: negative device %d for context %d", devices[k], k);
            return BBGPU_ERR_ARG;
        }
    // lock order of bbgpu_shutdown, which a failed binding ends in: the prover's mutex, then the library's
    std::lock_guard<std::mutex> lkp(plonk_mutex());
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (g_ctxs[0].ready) {
        bool same = g_num_ctx == count;
        for (int k = 0; same && k < count; k++) same = g_ctxs[k].device == devices[k];
        if (same) return BBGPU_OK;
        set_error("already bound to %d context(s), the first on device %d: bbgpu_shutdown() first", g_num_ctx, g_ctxs[0].device);
        return BBGPU_ERR_STATE;
    }
    const int cnt = hip_device_count();
    if (cnt == 0) {
        set_error("no HIP device available: the GPU entry points of libbbgpu have no CPU fallback");
        return BBGPU_ERR_HIP;
    }
    for (int k = 0; k < count; k++)
        if (devices[k] >= cnt) {
            set_error("bbgpu_init_devices: device %d of context %d, the machine has %d", devices[k], k, cnt);
            return BBGPU_ERR_ARG;
        }
    g_ctxs[0].device = devices[0];
    if (int rc = ensure_init()) return rc;
    for (int k = 1; k < count; k++) { // one after the other: each context's streams are made in one piece (ensure_init)
        g_ctxs[k].device = devices[k];
        g_workers[k] = new MultiWorker(k);
        g_num_ctx = k + 1;
        g_workers[k]->post([] { return ensure_init(); });
        char e[sizeof(g_err)];
        if (int rc = g_workers[k]->wait(e)) {
            shutdown_locked();
            e[sizeof(e) - 1] = 0;
            set_error("context %d (device %d): %s", k, devices[k], e);
            return rc;
        }
    }
    return BBGPU_OK;
}

int bbgpu_num_contexts(void)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return g_num_ctx;
}

void bbgpu_shutdown(void)
{
    // lock order: the prover's mutex, then the library's (the prover calls the entry points above while it holds its own)
    std::lock_guard<std::mutex> lkp(plonk_mutex());
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    shutdown_locked();
}

int bbgpu_memory_stats(bbgpu_memory_info* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!out) return BBGPU_ERR_ARG;
    memset(out, 0, sizeof(*out));
    for (int k = 0; k < g_num_ctx; k++) add_context_memory(g_ctxs[k], k == 0, out);
    return BBGPU_OK;
}

int bbgpu_memory_stats_context(int context, bbgpu_memory_info* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!out) {
        set_error("null output");
        return BBGPU_ERR_ARG;
    }
    if (context < 0 || context >= g_num_ctx) {
        set_error("no context %d (%d bound)", context, g_num_ctx);
        return BBGPU_ERR_ARG;
    }
    memset(out, 0, sizeof(*out));
    add_context_memory(g_ctxs[context], context == 0, out);
    return BBGPU_OK;
}

int bbgpu_fault_inject(const char* spec)
{
    if (fault_set(spec)) {
        set_error("fault spec '%s' not understood (alloc:k | h2d:k | d2h:k | launch:k)", spec ? spec : "");
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}
int bbgpu_fault_stats(bbgpu_fault_info* out)
{
    if (!out) return BBGPU_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    FaultState& F = fault();
    memset(out, 0, sizeof(*out));
    out->alloc_calls = F.calls[F_ALLOC].load();
    out->h2d_calls = F.calls[F_H2D].load();
    out->d2h_calls = F.calls[F_D2H].load();
    out->launch_checks = F.calls[F_LAUNCH].load();
    out->armed = F.armed_kind.load() >= 0 ? 1 : 0;
    out->fired = F.fired.load();
    out->absorbed = F.absorbed.load();
    {
        std::lock_guard<std::mutex> lf(F.mu);
        out->live_allocations = F.live.size();
        out->live_bytes = F.live_bytes;
    }
    for (int k = 0; k < g_num_ctx; k++)
        for (const auto& sl : g_ctxs[k].slot)
            if (sl.pending) out->slots_pending++;
    return BBGPU_OK;
}

void bbgpu_set_timing(int enabled)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    for (auto& C : g_ctxs) C.timing = enabled < 0 || enabled > 2 ? 1 : enabled; // settings apply to every context, bound or not
}
int bbgpu_last_timing(float* ms_out, int max_entries)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int k = ctx().last.count < max_entries ? ctx().last.count : max_entries;
    for (int i = 0; i < k; i++) ms_out[i] = ctx().last.ms[i];
    return k;
}

/* ---- NTT ---- */
int bbgpu_ntt_device(uint64_t* d_coeffs, size_t n, int kind, const uint64_t* constant, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    const int lg = log2_exact(n);
    if (lg < 1) {
        set_error("NTT size %zu is not a power of two >= 2", n);
        return BBGPU_ERR_SIZE;
    }
    if (kind < 0 || kind > BBGPU_COSET_FFT_WITH_CONSTANT || !d_coeffs) {
        set_error("bad NTT kind / null buffer");
        return BBGPU_ERR_ARG;
    }
    rc = grow(&ctx().d_scratch, &ctx().scratch_cap, n * 32);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream; /* NULL = the legacy default stream, as bbgpu.h says */
    if ((rc = shared_begin(st)) != BBGPU_OK) return rc;
    rc = ntt_device(d_coeffs, ctx().d_scratch, lg, kind, constant, st);
    if (rc == BBGPU_OK) rc = shared_end(st);
    if (rc == BBGPU_ERR_SIZE) set_error("NTT size 2^%d unsupported (max 2^28)", lg);
    if (rc == BBGPU_ERR_HIP) {
        const hipError_t he = hipGetLastError(); // hipSuccess: the failing call has already described itself (launch_check / dev_malloc)
        if (he != hipSuccess) set_error("NTT launch failed: %s", hipGetErrorString(he));
    }
    return rc;
}

int bbgpu_ntt_device_batch(uint64_t* d_coeffs, size_t n, size_t stride_elems, int batch, int kind, const uint64_t* constant, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    const int lg = log2_exact(n);
    if (lg < 1) {
        set_error("NTT size %zu is not a power of two >= 2", n);
        return BBGPU_ERR_SIZE;
    }
    if (kind < 0 || kind > BBGPU_COSET_FFT_WITH_CONSTANT || !d_coeffs || batch < 1 || batch > 64 || stride_elems < n) {
        set_error("bad NTT kind / null buffer / batch / stride");
        return BBGPU_ERR_ARG;
    }
    rc = grow(&ctx().d_scratch, &ctx().scratch_cap, (size_t)batch * n * 32);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream; /* NULL = the legacy default stream, as bbgpu.h says */
    if ((rc = shared_begin(st)) != BBGPU_OK) return rc;
    rc = ntt_device_batch(d_coeffs, stride_elems, batch, ctx().d_scratch, lg, kind, constant, st);
    if (rc == BBGPU_OK) rc = shared_end(st);
    if (rc == BBGPU_ERR_SIZE) set_error("NTT size 2^%d unsupported (max 2^28)", lg);
    if (rc == BBGPU_ERR_HIP) {
        const hipError_t he = hipGetLastError(); // hipSuccess: the failing call has already described itself (launch_check / dev_malloc)
        if (he != hipSuccess) set_error("NTT launch failed: %s", hipGetErrorString(he));
    }
    return rc;
}

int bbgpu_ntt(uint64_t* coeffs, size_t n, int kind, const uint64_t* constant)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!coeffs) return BBGPU_ERR_ARG;
    read_host_env();
    if (n <= (size_t)ctx().host_ntt_max && log2_exact(n) >= 1 && kind >= 0 && kind <= BBGPU_COSET_FFT_WITH_CONSTANT) {
        const bool has_const = (kind == BBGPU_FFT_WITH_CONSTANT || kind == BBGPU_IFFT_WITH_CONSTANT || kind == BBGPU_COSET_FFT_WITH_CONSTANT);
        if (has_const && !constant) return BBGPU_ERR_ARG;
        host::ntt_small(coeffs, log2_exact(n), kind, constant); // SURVEY 8b small sizes: no copy, no launch
        return BBGPU_OK;
    }
    int rc = ensure_init();
    if (rc) return rc;
    rc = grow(&ctx().d_stage, &ctx().stage_cap, n * 32);
    if (rc) return rc;
    if ((rc = host_to_device(ctx().d_stage, coeffs, n * 32, ctx().stream)) != BBGPU_OK) return rc;
    rc = bbgpu_ntt_device(ctx().d_stage, n, kind, constant, ctx().stream);
    if (rc) return rc;
    // up to here `coeffs` is untouched; a failure while the result is copied back may leave it half overwritten -- LOST only if a byte of it was written
    bool touched = false;
    rc = device_to_host_sync(coeffs, ctx().d_stage, n * 32, ctx().stream, &touched);
    return rc == BBGPU_OK ? BBGPU_OK : (touched ? BBGPU_ERR_LOST : rc);
}

/* ---- resident polynomial helpers ---- */
struct SharedGuard { // records "this stream is done with the shared workspaces" on every way out of a helper
    hipStream_t st;
    ~SharedGuard() { (void)shared_end(st); }
};
#define POLY_ENTER(ptr_ok)                                                                                              \
    std::lock_guard<std::recursive_mutex> lk(g_mu);                                                                     \
    {                                                                                                                   \
        int rc_ = ensure_init();                                                                                        \
        if (rc_) return rc_;                                                                                            \
        if (!(ptr_ok)) {                                                                                                \
            set_error("null device pointer");                                                                           \
            return BBGPU_ERR_ARG;                                                                                       \
        }                                                                                                               \
    }                                                                                                                   \
    hipStream_t st = (hipStream_t)hip_stream; /* NULL = the legacy default stream, as bbgpu.h says */                                               \
    if (int rcb_ = shared_begin(st)) return rcb_;                                                                       \
    SharedGuard shared_guard_{ st }

static host::Fr load_fr(const uint64_t z[4])
{
    host::Fr r;
    memcpy(r.d, z, 32);
    return r;
}

int bbgpu_fr_evaluate_device(const uint64_t* d_coeffs, size_t n, const uint64_t z[4], uint64_t out[4], void* hip_stream)
{
    POLY_ENTER((d_coeffs || n == 0) && z && out);
    host::Fr r;
    int rc = poly::evaluate(d_coeffs, n, load_fr(z), &r, ctx().poly_scratch, st);
    if (rc) return rc;
    memcpy(out, r.d, 32);
    return BBGPU_OK;
}

int bbgpu_fr_batch_invert_device(uint64_t* d_values, size_t n, void* hip_stream)
{
    POLY_ENTER(d_values || n == 0);
    int rc = grow(&ctx().d_poly_tmp, &ctx().poly_tmp_cap, n * 32);
    if (rc) return rc;
    return poly::batch_invert(d_values, ctx().d_poly_tmp, n, ctx().poly_scratch, st);
}

int bbgpu_fr_product_scan_device(const uint64_t* d_in, uint64_t* d_out, size_t n, int reverse, int inclusive, void* hip_stream)
{
    POLY_ENTER((d_in && d_out) || n == 0);
    return poly::product_scan(d_in, d_out, n, reverse != 0, inclusive != 0, ctx().poly_scratch, st, nullptr);
}

int bbgpu_fr_mul_device(uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t n, void* hip_stream)
{
    POLY_ENTER((d_out && d_a && d_b) || n == 0);
    return poly::mul_pointwise(d_out, d_a, d_b, n, st);
}

int bbgpu_kate_opening_device(const uint64_t* d_src, uint64_t* d_dest, size_t n, const uint64_t z[4], uint64_t f_of_z[4], void* hip_stream)
{
    POLY_ENTER(((d_src && d_dest) || n == 0) && z);
    const host::Fr zz = load_fr(z);
    if (f_of_z) {
        host::Fr f;
        int rc = poly::evaluate(d_src, n, zz, &f, ctx().poly_scratch, st);
        if (rc) return rc;
        memcpy(f_of_z, f.d, 32);
    }
    const uint64_t* src = d_src;
    if (d_dest == d_src) { // the scan's last phase reads its input while writing: work from a copy
        int rc = grow(&ctx().d_poly_tmp, &ctx().poly_tmp_cap, n * 32);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx().d_poly_tmp, d_src, n * 32, hipMemcpyDeviceToDevice, st));
        src = ctx().d_poly_tmp;
    }
    return poly::horner_suffix(src, d_dest, n, zz, false, ctx().poly_scratch, st, nullptr);
}

/* ---- evaluation and opening in evaluation form (host_lagrange_open.hpp, poly.hip bary_open) ---- */
// the verdict both the device entries and the host twins give on their arguments; ptr_ok: the entry's own pointers
static int lagrange_open_args(const char* what, bool ptr_ok, size_t n, size_t stride_elems, int batch)
{
    if (!host::lagrange_open_sizes_ok(n, stride_elems, batch)) {
        set_error("%s: n = %zu must be a power of two in [2, 2^%d], batch = %d in 1..%d and the stride (%zu) no smaller than n", what, n,
                  host::LAGRANGE_OPEN_MAX_LOG2, batch, host::LAGRANGE_OPEN_MAX_BATCH, stride_elems);
        return BBGPU_ERR_SIZE;
    }
    if (!ptr_ok) {
        set_error("%s: null values / quotient / z / out", what);
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}
// argument errors are refused before a device is bound; the case decision (z on the domain, and where) is the host's, before anything is launched
static int lagrange_open_device(const char* what, bool ptr_ok, const uint64_t* d_values, uint64_t* d_quotient, size_t n, size_t stride_elems, int batch,
                                const uint64_t* z, uint64_t* out, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rc = lagrange_open_args(what, ptr_ok, n, stride_elems, batch)) return rc;
    if (int rc = ensure_init()) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = shared_begin(st)) return rc;
    SharedGuard shared_guard_{ st };
    const int log2n = host::lagrange_open_log2(n);
    const host::Fr zz = host::fr_mul(load_fr(z), host::fr_one());
    size_t m = 0;
    const bool on = host::lagrange_open_on_domain(zz, log2n, &m);
    if (!on || d_quotient)
        if (int rc = grow(&ctx().d_poly_tmp, &ctx().poly_tmp_cap, n * 32)) return rc;
    std::vector<host::Fr> y(out ? (size_t)batch : 0);
    if (int rc = poly::bary_open(d_values, d_quotient, log2n, stride_elems, batch, zz, on, m, ctx().d_poly_tmp, out ? y.data() : nullptr, ctx().poly_scratch, st))
        return rc;
    if (out) memcpy(out, y.data(), (size_t)batch * 32);
    return BBGPU_OK;
}
int bbgpu_fr_evaluate_lagrange_device(const uint64_t* d_values, size_t n, size_t stride_elems, int batch, const uint64_t z[4], uint64_t* out, void* hip_stream)
{
    return lagrange_open_device("evaluate_lagrange", d_values && z && out, d_values, nullptr, n, stride_elems, batch, z, out, hip_stream);
}
int bbgpu_kate_opening_lagrange_device(const uint64_t* d_values, uint64_t* d_quotient, size_t n, size_t stride_elems, int batch, const uint64_t z[4],
                                       uint64_t* f_of_z, void* hip_stream)
{
    return lagrange_open_device("kate_opening_lagrange", d_values && d_quotient && z, d_values, d_quotient, n, stride_elems, batch, z, f_of_z, hip_stream);
}

/* ---- opening sessions: several points over ONE shared inversion, folded openings (poly.hip bary_inverses / bary_open_with / bary_open_folded) ---- */
int bbgpu_lagrange_opening_begin(size_t n, const uint64_t* z, int points, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const int log2n = host::lagrange_open_log2(n);
    if (log2n < 1 || points < 1 || points > BBGPU_OPENING_MAX_POINTS || (size_t)points * n > ((size_t)1 << host::LAGRANGE_OPEN_MAX_LOG2)) {
        set_error("lagrange_opening_begin: n = %zu must be a power of two in [2, 2^%d], points = %d in 1..%d and points x n at most 2^%d", n,
                  host::LAGRANGE_OPEN_MAX_LOG2, points, BBGPU_OPENING_MAX_POINTS, host::LAGRANGE_OPEN_MAX_LOG2);
        return BBGPU_ERR_SIZE;
    }
    if (!z) {
        set_error("lagrange_opening_begin: null z");
        return BBGPU_ERR_ARG;
    }
    int slot = -1;
    for (int k = 0; k < BBGPU_OPENING_MAX_SESSIONS && slot < 0; k++)
        if (!g_opening[k].live) slot = k;
    if (slot < 0) {
        set_error("lagrange_opening_begin: %d sessions are live", BBGPU_OPENING_MAX_SESSIONS);
        return BBGPU_ERR_STATE;
    }
    if (int rc = ensure_init()) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = shared_begin(st)) return rc;
    SharedGuard shared_guard_{ st };
    OpeningSession o;
    o.log2n = log2n;
    o.points = points;
    for (int t = 0; t < points; t++) {
        o.z[t] = host::fr_mul(load_fr(z + 4 * t), host::fr_one());
        o.m[t] = 0;
        o.on[t] = host::lagrange_open_on_domain(o.z[t], log2n, &o.m[t]);
    }
    o.bytes = (size_t)points * n * 32;
    if (int rc = grow(&ctx().d_poly_tmp, &ctx().poly_tmp_cap, o.bytes)) return rc;
    HIPCHK(dev_malloc((void**)&o.d_inv, o.bytes));
    if (int rc = poly::bary_inverses(o.d_inv, log2n, points, o.z, o.on, o.m, ctx().d_poly_tmp, ctx().poly_scratch, st)) {
        (void)dev_free(o.d_inv); // (waits for the device: nothing queued still writes it)
        return rc;
    }
    o.live = true;
    g_opening[slot] = o;
    return slot;
}
// the verdict the session calls share, in this order: batch, the call's own pointers, the session and its point, the stride (against the session's n)
static int opening_call_args(const char* what, int session, int point, bool ptr_ok, size_t stride_elems, int batch, OpeningSession** out)
{
    if (batch < 1 || batch > host::LAGRANGE_OPEN_MAX_BATCH) {
        set_error("%s: batch = %d must be in 1..%d", what, batch, host::LAGRANGE_OPEN_MAX_BATCH);
        return BBGPU_ERR_SIZE;
    }
    if (!ptr_ok) {
        set_error("%s: null values / quotient / gamma / out", what);
        return BBGPU_ERR_ARG;
    }
    if (session < 0 || session >= BBGPU_OPENING_MAX_SESSIONS || !g_opening[session].live) {
        set_error("%s: unknown opening session %d", what, session);
        return BBGPU_ERR_ARG;
    }
    OpeningSession& o = g_opening[session];
    if (point < 0 || point >= o.points) {
        set_error("%s: point %d, the session has %d", what, point, o.points);
        return BBGPU_ERR_ARG;
    }
    if (stride_elems < ((size_t)1 << o.log2n)) {
        set_error("%s: the stride (%zu) is smaller than n = %zu", what, stride_elems, (size_t)1 << o.log2n);
        return BBGPU_ERR_SIZE;
    }
    *out = &o;
    return BBGPU_OK;
}
static int opening_session_open(const char* what, bool ptr_ok, int session, int point, const uint64_t* d_values, uint64_t* d_quotient, size_t stride_elems,
                                int batch, uint64_t* out, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    OpeningSession* o = nullptr;
    if (int rc = opening_call_args(what, session, point, ptr_ok, stride_elems, batch, &o)) return rc;
    if (int rc = ensure_init()) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = shared_begin(st)) return rc;
    SharedGuard shared_guard_{ st };
    std::vector<host::Fr> y(out ? (size_t)batch : 0);
    if (int rc = poly::bary_open_with(d_values, d_quotient, o->log2n, stride_elems, batch, o->z[point], o->on[point], o->m[point],
                                      o->d_inv + ((size_t)point << o->log2n) * 4, out ? y.data() : nullptr, ctx().poly_scratch, st))
        return rc;
    if (out) memcpy(out, y.data(), (size_t)batch * 32);
    return BBGPU_OK;
}
int bbgpu_lagrange_opening_evaluate(int session, int point, const uint64_t* d_values, size_t stride_elems, int batch, uint64_t* out, void* hip_stream)
{
    return opening_session_open("lagrange_opening_evaluate", d_values && out, session, point, d_values, nullptr, stride_elems, batch, out, hip_stream);
}
int bbgpu_lagrange_opening_open(int session, int point, const uint64_t* d_values, uint64_t* d_quotient, size_t stride_elems, int batch, uint64_t* f_of_z,
                                void* hip_stream)
{
    return opening_session_open("lagrange_opening_open", d_values && d_quotient, session, point, d_values, d_quotient, stride_elems, batch, f_of_z, hip_stream);
}
int bbgpu_lagrange_opening_open_folded(int session, int point, const uint64_t* d_values, size_t stride_elems, int batch, const uint64_t* gamma,
                                       uint64_t* d_quotient, int accumulate, uint64_t folded_f_of_z[4], void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    OpeningSession* o = nullptr;
    if (int rc = opening_call_args("lagrange_opening_open_folded", session, point, d_values && d_quotient && gamma, stride_elems, batch, &o)) return rc;
    if (int rc = ensure_init()) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = shared_begin(st)) return rc;
    SharedGuard shared_guard_{ st };
    std::vector<host::Fr> g((size_t)batch);
    for (int b = 0; b < batch; b++) g[b] = load_fr(gamma + 4 * b);
    host::Fr f;
    if (int rc = poly::bary_open_folded(d_values, o->log2n, stride_elems, batch, g.data(), o->z[point], o->on[point], o->m[point],
                                        o->d_inv + ((size_t)point << o->log2n) * 4, d_quotient, accumulate != 0, folded_f_of_z ? &f : nullptr,
                                        ctx().poly_scratch, st))
        return rc;
    if (folded_f_of_z) memcpy(folded_f_of_z, f.d, 32);
    return BBGPU_OK;
}
int bbgpu_lagrange_opening_end(int session)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (session < 0 || session >= BBGPU_OPENING_MAX_SESSIONS || !g_opening[session].live) {
        set_error("lagrange_opening_end: unknown opening session %d", session);
        return BBGPU_ERR_ARG;
    }
    opening_release(g_opening[session]); // (dev_free waits for the device: no queued call still reads the inverses)
    return BBGPU_OK;
}

// the verdict of the fold and its twin
static int fold_args(const char* what, bool ptr_ok, size_t n, size_t stride_elems, int batch)
{
    if (!host::fold_sizes_ok(n, stride_elems, batch)) {
        set_error("%s: n = %zu must be in [1, 2^24], batch = %d in 1..%d and the stride (%zu) no smaller than n", what, n, batch, host::LAGRANGE_OPEN_MAX_BATCH,
                  stride_elems);
        return BBGPU_ERR_SIZE;
    }
    if (!ptr_ok) {
        set_error("%s: null out / values / gamma", what);
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}
int bbgpu_fr_fold_device(uint64_t* d_out, const uint64_t* d_values, size_t n, size_t stride_elems, int batch, const uint64_t* gamma, int accumulate,
                         void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rc = fold_args("fr_fold", d_out && d_values && gamma, n, stride_elems, batch)) return rc;
    if (int rc = ensure_init()) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = shared_begin(st)) return rc;
    SharedGuard shared_guard_{ st };
    std::vector<host::Fr> g((size_t)batch);
    for (int b = 0; b < batch; b++) g[b] = load_fr(gamma + 4 * b);
    return poly::fold(d_out, d_values, n, stride_elems, batch, g.data(), accumulate != 0, st);
}

int bbgpu_lagrange_l1_fft_device(uint64_t* d_l_1, size_t n_src, size_t n_target, void* hip_stream)
{
    POLY_ENTER(d_l_1);
    const int ls = log2_exact(n_src), lt = log2_exact(n_target);
    if (ls < 1 || lt < ls || lt > 28) {
        set_error("lagrange_l1_fft: domains must be powers of two, target >= source");
        return BBGPU_ERR_SIZE;
    }
    int rc = grow(&ctx().d_poly_tmp, &ctx().poly_tmp_cap, n_target * 32);
    if (rc) return rc;
    return poly::lagrange_l1_fft(d_l_1, ctx().d_poly_tmp, ls, lt, ctx().poly_scratch, st);
}

int bbgpu_divide_by_pseudo_vanishing_device(uint64_t* d_coeffs, size_t n_src, size_t n_target, void* hip_stream)
{
    POLY_ENTER(d_coeffs);
    const int ls = log2_exact(n_src), lt = log2_exact(n_target);
    if (ls < 1 || lt < ls || lt > 28) {
        set_error("divide_by_pseudo_vanishing: domains must be powers of two, target >= source");
        return BBGPU_ERR_SIZE;
    }
    return poly::divide_by_pseudo_vanishing(d_coeffs, ls, lt, st);
}

int bbgpu_permutation_lagrange_base_device(uint64_t* d_out, const uint32_t* d_mapping, size_t n, void* hip_stream)
{
    POLY_ENTER(d_out && d_mapping);
    const int lg = log2_exact(n);
    if (lg < 1 || lg > 28) return BBGPU_ERR_SIZE;
    int rc = grow(&ctx().d_poly_tmp, &ctx().poly_tmp_cap, n * 32);
    if (rc) return rc;
    rc = poly::powers(ctx().d_poly_tmp, n, host::fr_root_of_unity(lg), host::fr_one(), st);
    if (rc) return rc;
    return poly::sigma_from_mapping(d_out, d_mapping, ctx().d_poly_tmp, n, st);
}

/* ---- the same helpers on host buffers (what the C++ shim forwards the reference's co-resident TU functions to) ---- */
static int stage_in(const uint64_t* host, size_t n)
{
    int rc = grow(&ctx().d_stage, &ctx().stage_cap, n * 32);
    if (rc) return rc;
    return host_to_device(ctx().d_stage, host, n * 32, ctx().stream);
}
// in_place: the destination is also the call's input -- a failure after any byte of it was written is BBGPU_ERR_LOST (nothing left to fall back on)
static int stage_out(uint64_t* host, const uint64_t* dev, size_t n, bool in_place = false)
{
    bool touched = false;
    const int rc = device_to_host_sync(host, dev, n * 32, ctx().stream, &touched);
    return (rc != BBGPU_OK && in_place && touched) ? BBGPU_ERR_LOST : rc;
}

int bbgpu_fr_evaluate(const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t out[4])
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    if ((!coeffs && n) || !z || !out) return BBGPU_ERR_ARG;
    if ((rc = stage_in(coeffs, n)) != BBGPU_OK) return rc;
    return bbgpu_fr_evaluate_device(ctx().d_stage, n, z, out, ctx().stream);
}

int bbgpu_kate_opening(const uint64_t* src, uint64_t* dest, size_t n, const uint64_t z[4], uint64_t f_of_z[4])
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    if (((!src || !dest) && n) || !z) return BBGPU_ERR_ARG;
    if ((rc = stage_in(src, n)) != BBGPU_OK) return rc;
    if ((rc = grow(&ctx().d_stage2, &ctx().stage2_cap, n * 32)) != BBGPU_OK) return rc;
    if ((rc = bbgpu_kate_opening_device(ctx().d_stage, ctx().d_stage2, n, z, f_of_z, ctx().stream)) != BBGPU_OK) return rc;
    // the reference calls it in place (polynomial.cpp:327 passes coefficients, coefficients): then a half-written dest is a half-destroyed src
    return stage_out(dest, ctx().d_stage2, n, dest == src);
}

int bbgpu_lagrange_l1_fft(uint64_t* l_1, size_t n_src, size_t n_target)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    if (!l_1) return BBGPU_ERR_ARG;
    if ((rc = grow(&ctx().d_stage, &ctx().stage_cap, n_target * 32)) != BBGPU_OK) return rc;
    if ((rc = bbgpu_lagrange_l1_fft_device(ctx().d_stage, n_src, n_target, ctx().stream)) != BBGPU_OK) return rc;
    return stage_out(l_1, ctx().d_stage, n_target);
}

int bbgpu_divide_by_pseudo_vanishing(uint64_t* coeffs, size_t n_src, size_t n_target)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    if (!coeffs) return BBGPU_ERR_ARG;
    if ((rc = stage_in(coeffs, n_target)) != BBGPU_OK) return rc;
    if ((rc = bbgpu_divide_by_pseudo_vanishing_device(ctx().d_stage, n_src, n_target, ctx().stream)) != BBGPU_OK) return rc;
    return stage_out(coeffs, ctx().d_stage, n_target, true); // in place, as in bbgpu_ntt
}

// polynomial_arithmetic::get_lagrange_evaluations (polynomial_arithmetic.cpp:594-626): {Z_H*(z), L_1(z), L_{n-1}(z)}; host arithmetic
int bbgpu_lagrange_evaluations(const uint64_t z[4], size_t n, uint64_t out[12])
{
    const int lg = log2_exact(n);
    if (!z || !out || lg < 1) return BBGPU_ERR_ARG;
    const host::Fr zc = load_fr(z), one = host::fr_one(), root = host::fr_root_of_unity(lg), root_inv = host::fr_inv(root);
    host::Fr zp = zc;
    for (int i = 0; i < lg; i++) zp = host::fr_sqr(zp);
    const host::Fr numerator = host::fr_sub(zp, one);
    const host::Fr d0 = host::fr_inv(host::fr_sub(zc, root_inv)), d1 = host::fr_inv(host::fr_sub(zc, one));
    const host::Fr d2 = host::fr_inv(host::fr_sub(host::fr_mul(host::fr_mul(zc, root), root), one));
    const host::Fr scaled = host::fr_mul(numerator, host::fr_inv(host::fr_from_u64((uint64_t)n)));
    const host::Fr v = host::fr_mul(numerator, d0), l1 = host::fr_mul(scaled, d1), ln = host::fr_mul(scaled, d2);
    memcpy(out, v.d, 32);
    memcpy(out + 4, l1.d, 32);
    memcpy(out + 8, ln.d, 32);
    return BBGPU_OK;
}

// scalar_multiplication::generate_pippenger_point_table (scalar_multiplication.cpp:131-140): table[2i] = P_i, table[2i+1] = (beta x_i, -y_i),
// filled from the back so that `points` may alias `table`.  Host arithmetic (once per SRS).
int bbgpu_generate_point_table(const uint64_t* points, uint64_t* table, size_t n)
{
    if ((!points || !table) && n) return BBGPU_ERR_ARG;
    const host::Fq beta = { { 0x71930c11d782e155ULL, 0xa6bb947cffbe3323ULL, 0xaa303344d4741444ULL, 0x2c3b3f0d26594943ULL } }; // fq.hpp:53-56
    const host::Fq zero = { { 0, 0, 0, 0 } };
    for (size_t i = n; i-- > 0;) {
        host::Fq x, y;
        memcpy(x.d, points + i * 8, 32);
        memcpy(y.d, points + i * 8 + 4, 32);
        const host::Fq bx = host::fq_mul(x, beta), ny = host::fq_sub(zero, y);
        uint64_t* e = table + i * 16;
        memcpy(e + 8, bx.d, 32);
        memcpy(e + 12, ny.d, 32);
        memcpy(e, x.d, 32);
        memcpy(e + 4, y.d, 32);
    }
    return BBGPU_OK;
}

/* ---- host fallbacks: what shim/bb_shim.cpp computes with after a GPU entry has FAILED (host_fallback.hpp).  No HIP call, no lock,
 * no shared state: re-entrant.  Never reached from the GPU entries above. ---- */
int bbgpu_host_msm_g1(const uint64_t* scalars, const uint64_t* points, size_t n, int plain_table, uint64_t out[12])
{
    if (!out || (n && (!scalars || !points))) {
        set_error("null scalars / points / out");
        return BBGPU_ERR_ARG;
    }
    host::g1_to_normalised(host::msm_pippenger(scalars, points, n, plain_table ? 8 : 16), out);
    return BBGPU_OK;
}
int bbgpu_host_ntt(uint64_t* coeffs, size_t n, int kind, const uint64_t* constant)
{
    const int lg = log2_exact(n);
    if (lg < 1 || lg > 28) {
        set_error("NTT size %zu is not a power of two in [2, 2^28]", n);
        return BBGPU_ERR_SIZE;
    }
    const bool has_const = (kind == BBGPU_FFT_WITH_CONSTANT || kind == BBGPU_IFFT_WITH_CONSTANT || kind == BBGPU_COSET_FFT_WITH_CONSTANT);
    if (!coeffs || kind < 0 || kind > BBGPU_COSET_FFT_WITH_CONSTANT || (has_const && !constant)) {
        set_error("bad NTT kind / null buffer");
        return BBGPU_ERR_ARG;
    }
    host::ntt_radix2(coeffs, lg, kind, constant);
    return BBGPU_OK;
}
int bbgpu_host_fr_evaluate(const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t out[4])
{
    if ((!coeffs && n) || !z || !out) return BBGPU_ERR_ARG;
    const host::Fr r = host::poly_evaluate(coeffs, n, load_fr(z));
    memcpy(out, r.d, 32);
    return BBGPU_OK;
}
int bbgpu_host_kate_opening(const uint64_t* src, uint64_t* dest, size_t n, const uint64_t z[4], uint64_t f_of_z[4])
{
    if (((!src || !dest) && n) || !z) return BBGPU_ERR_ARG;
    const host::Fr f = host::kate_opening(src, dest, n, load_fr(z));
    if (f_of_z) memcpy(f_of_z, f.d, 32);
    return BBGPU_OK;
}
int bbgpu_host_fr_evaluate_lagrange(const uint64_t* values, size_t n, size_t stride_elems, int batch, const uint64_t z[4], uint64_t* out)
{
    if (int rc = lagrange_open_args("host evaluate_lagrange", values && z && out, n, stride_elems, batch)) return rc;
    host::lagrange_open_host(values, nullptr, n, stride_elems, batch, load_fr(z), out);
    return BBGPU_OK;
}
int bbgpu_host_kate_opening_lagrange(const uint64_t* values, uint64_t* quotient, size_t n, size_t stride_elems, int batch, const uint64_t z[4],
                                     uint64_t* f_of_z)
{
    if (int rc = lagrange_open_args("host kate_opening_lagrange", values && quotient && z, n, stride_elems, batch)) return rc;
    host::lagrange_open_host(values, quotient, n, stride_elems, batch, load_fr(z), f_of_z);
    return BBGPU_OK;
}
int bbgpu_host_fr_fold(uint64_t* out, const uint64_t* values, size_t n, size_t stride_elems, int batch, const uint64_t* gamma, int accumulate)
{
    if (int rc = fold_args("host fr_fold", out && values && gamma, n, stride_elems, batch)) return rc;
    host::fold_host(out, values, n, stride_elems, batch, gamma, accumulate != 0);
    return BBGPU_OK;
}
int bbgpu_host_kate_opening_lagrange_folded(const uint64_t* values, size_t n, size_t stride_elems, int batch, const uint64_t* gamma, const uint64_t z[4],
                                            uint64_t* quotient, int accumulate, uint64_t folded_f_of_z[4])
{
    if (int rc = lagrange_open_args("host kate_opening_lagrange_folded", values && gamma && z && quotient, n, stride_elems, batch)) return rc;
    host::lagrange_open_folded_host(values, n, stride_elems, batch, gamma, load_fr(z), quotient, accumulate != 0, folded_f_of_z);
    return BBGPU_OK;
}
int bbgpu_host_lagrange_l1_fft(uint64_t* l_1, size_t n_src, size_t n_target)
{
    const int ls = log2_exact(n_src), lt = log2_exact(n_target);
    if (!l_1) return BBGPU_ERR_ARG;
    if (ls < 1 || lt < ls || lt > 28) return BBGPU_ERR_SIZE;
    host::lagrange_l1_fft(l_1, ls, lt);
    return BBGPU_OK;
}
int bbgpu_host_divide_by_pseudo_vanishing(uint64_t* coeffs, size_t n_src, size_t n_target)
{
    const int ls = log2_exact(n_src), lt = log2_exact(n_target);
    if (!coeffs) return BBGPU_ERR_ARG;
    if (ls < 1 || lt < ls || lt > 28) return BBGPU_ERR_SIZE;
    host::divide_by_pseudo_vanishing(coeffs, ls, lt);
    return BBGPU_OK;
}

/* ---- the pairing and the SRS check (host_pairing.hpp, host_srs_check.hpp, srs_check.hip) ---- */
int bbgpu_host_pairing(const uint64_t p[8], const uint64_t q[16], uint64_t out[48])
{
    if (!p || !q || !out) {
        set_error("null p / q / out");
        return BBGPU_ERR_ARG;
    }
    const host::Fq12 e = host::pairing_product(p, q, 1);
    memcpy(out, &e, 384);
    return BBGPU_OK;
}
int bbgpu_host_pairing_check(const uint64_t* p, const uint64_t* q, size_t k, int* is_one)
{
    if (!is_one || (k && (!p || !q))) {
        set_error("null p / q / is_one");
        return BBGPU_ERR_ARG;
    }
    *is_one = host::fq12_eq(host::pairing_product(p, q, k), host::fq12_one()) ? 1 : 0;
    return BBGPU_OK;
}

int bbgpu_host_kzg_check_openings(const uint64_t* commitments, const uint64_t* z, const uint64_t* y, const uint64_t* proofs, size_t k, const uint64_t g2_x[16],
                                  const uint64_t seed[4], int* ok)
{
    if (k < 1 || k > host::KZG_CHECK_MAX_OPENINGS) {
        set_error("KZG check: %zu openings, 1..%zu are taken", k, host::KZG_CHECK_MAX_OPENINGS);
        return BBGPU_ERR_SIZE;
    }
    if (!commitments || !z || !y || !proofs || !g2_x || !ok) {
        set_error("KZG check: null commitments / z / y / proofs / g2_x / ok");
        return BBGPU_ERR_ARG;
    }
    for (size_t t = 0; t < k; t++)
        if (!host::g1_words_acceptable(commitments + 8 * t) || !host::g1_words_acceptable(proofs + 8 * t)) {
            set_error("KZG check: commitment or proof %zu is not on the curve", t);
            return BBGPU_ERR_ARG;
        }
    if (!host::srs_check_g2_ok(g2_x)) {
        set_error("KZG check: g2_x is at infinity, off the twist curve or not of order r");
        return BBGPU_ERR_ARG;
    }
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    // the batch check's twin over a call with one commitment per claim
    host::KzgCheckCall K;
    K.commitments = commitments;
    K.z = z;
    K.y = y;
    K.proofs = proofs;
    K.count = k;
    bbgpu_kzg_check_report rep;
    const int rc = host::kzg_check_host(K, g2_x, sd, 0, &rep);
    *ok = rep.ok ? 1 : 0;
    return rc;
}

// io.hpp:100-135,171-180 restated: behind the manifest's num_g1_points G1 records come num_g2_points G2 records of 128 bytes (x.c0, x.c1, y.c0, y.c1 in the
// format of the G1 coordinates); record 0 is the generator, record 1 is x * G2.  Host only.
int bbgpu_transcript_read_g2(const char* path, uint64_t g2_x_out[16])
{
    if (!path || !g2_x_out) return BBGPU_ERR_ARG;
    FILE* f = fopen(path, "rb");
    if (!f) {
        set_error("cannot open transcript %s", path);
        return BBGPU_ERR_ARG;
    }
    unsigned char man[28], rec[128];
    bool ok = fread(man, 1, 28, f) == 28;
    auto be32 = [&](int i) { return ((uint32_t)man[4 * i] << 24) | ((uint32_t)man[4 * i + 1] << 16) | ((uint32_t)man[4 * i + 2] << 8) | man[4 * i + 3]; };
    if (ok && be32(5) < 2) {
        fclose(f);
        set_error("transcript %s holds %u G2 points, x * G2 is the second", path, be32(5));
        return BBGPU_ERR_SIZE;
    }
    ok = ok && fseek(f, 28 + (long)be32(4) * 64 + 128, SEEK_SET) == 0 && fread(rec, 1, 128, f) == 128;
    fclose(f);
    if (!ok) {
        set_error("transcript %s: short read", path);
        return BBGPU_ERR_SIZE;
    }
    const host::Fq rsq = { { 0xF32CFC5B538AFA89ULL, 0xB5E71911D44501FBULL, 0x47AB1EFF0A417FF6ULL, 0x06D89F71CAB8351FULL } }; // 2^512 mod q (fq.hpp:48-51)
    for (int c = 0; c < 4; c++) {
        host::Fq v;
        for (int l = 0; l < 4; l++) {
            uint64_t w = 0;
            for (int b = 0; b < 8; b++) w = (w << 8) | rec[c * 32 + l * 8 + b];
            v.d[l] = w;
        }
        v = host::fq_mul(v, rsq);
        memcpy(g2_x_out + 4 * c, v.d, 32);
    }
    return BBGPU_OK;
}

int bbgpu_host_srs_check(const uint64_t* points_endo_table, size_t n, const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_srs_report* out)
{
    if (!points_endo_table || !out || n == 0 || (flags & ~BBGPU_SRS_CHECK_LOCATE)) {
        set_error("SRS check: null table / out, n == 0 or unknown flag bits 0x%x", flags);
        return BBGPU_ERR_ARG;
    }
    uint64_t sd[4];
    if (int rc = call_seed("SRS check", seed, sd)) return rc;
    return host::srs_check_host(points_endo_table, n, g2_x, sd, flags, out);
}

int bbgpu_srs_check(int srs_handle, size_t n, const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_srs_report* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound: a handle can only exist once one is
    if (!out || n == 0 || (flags & ~BBGPU_SRS_CHECK_LOCATE)) {
        set_error("SRS check: null out, n == 0 or unknown flag bits 0x%x", flags);
        return BBGPU_ERR_ARG;
    }
    const SrsEntry* ep = nullptr;
    if (int rc = srs_rows("SRS check", srs_handle, n, BBGPU_ERR_ARG, &ep)) return rc;
    if (int rc = ensure_init()) return rc;
    const SrsEntry& e = *ep;
    uint64_t sd[4];
    if (int rc = call_seed("SRS check", seed, sd)) return rc;
    host::srs_report_init(out, n, sd);
    out->g2_ok = host::srs_check_g2_ok(g2_x) ? 1 : 0;
    const bool want_powers = out->g2_ok && n >= 2;
    // one pass over the rows (row 0 against the generator (1, 2)) and, beside it, the multipliers; ONE synchronisation before the verdict on the curve test is read
    uint64_t gen256[8], gen[8], *d_rho = nullptr;
    host::g1_generator_words(gen256);
    resident_row(gen256, gen);
    if (int rc = curve_pass(e.d_srs, n, gen, want_powers ? (n - 1) * 32 : 0, 1, [&](uint64_t* d_extra, hipStream_t st) {
            d_rho = d_extra;
            return want_powers ? srs_check_scalars(sd, n - 1, d_rho, st) : (int)BBGPU_OK;
        }, &out->bad_points, &out->first_bad_point, &out->first_is_generator))
        return rc;
    if (!want_powers || out->bad_points) return BBGPU_OK;
    // A and B over the SAME scalars, against points [0, m) and [1, m + 1) of the handle
    return host::srs_check_powers(out, g2_x, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) { return two_msms(e, 0, d_rho, m, e, 1, d_rho, m, a12, b12); });
}

/* ---- batched PLONK verification (host_plonk_verify.hpp, plonk_verify.hip) ---- */
static int verify_args(const uint64_t* proofs, size_t count, int flags, const uint32_t* status, const bbgpu_plonk_verify_report* out)
{
    if (!proofs || !status || !out || count < 1 || (flags & ~BBGPU_PLONK_VERIFY_LOCATE)) {
        set_error("PLONK verify: null proofs / status / out, count < 1 or unknown flag bits 0x%x", flags);
        return BBGPU_ERR_ARG;
    }
    if (count > BBGPU_PLONK_VERIFY_MAX_BATCH) {
        set_error("PLONK verify: %zu proofs, at most %d per call", count, BBGPU_PLONK_VERIFY_MAX_BATCH);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}

int bbgpu_host_plonk_verify_batch(size_t n, int widgets, const uint64_t* vk, const uint64_t g2_x[16], const uint64_t* proofs, size_t count,
                                  const uint64_t seed[4], int flags, uint32_t* status, bbgpu_plonk_verify_report* out)
{
    if (int rc = verify_args(proofs, count, flags, status, out)) return rc;
    host::VerifyKey K;
    const char* why = "";
    if (int rc = host::verify_key_init(&K, n, widgets, vk, g2_x, &why)) {
        set_error("PLONK verify: %s", why);
        return rc;
    }
    uint64_t sd[4];
    if (int rc = call_seed("PLONK verify", seed, sd)) return rc;
    return host::verify_host(K, proofs, count, sd, flags, status, out);
}

// what bbgpu_plonk_verify_multi and its host twin refuse alike: `what` names the first argument ("verifiers" / "keys")
static int verify_multi_args(const void* circuits, int num, const char* what, const uint32_t* circuit, const uint64_t* proofs, size_t count, int flags,
                             const uint32_t* status, const bbgpu_plonk_verify_report* out)
{
    if (!circuits || !circuit) {
        set_error("PLONK verify: null %s or circuit", what);
        return BBGPU_ERR_ARG;
    }
    if (num < 1) {
        set_error("PLONK verify: %d %s, at least one", num, what);
        return BBGPU_ERR_ARG;
    }
    if (int rc = verify_args(proofs, count, flags, status, out)) return rc;
    if (num > BBGPU_PLONK_VERIFY_MAX_CIRCUITS) {
        set_error("PLONK verify: %d %s, at most %d per call", num, what, BBGPU_PLONK_VERIFY_MAX_CIRCUITS);
        return BBGPU_ERR_SIZE;
    }
    for (size_t j = 0; j < count; j++)
        if (circuit[j] >= (uint32_t)num) {
            set_error("PLONK verify: circuit[%zu] = %u, but there are %d %s", j, circuit[j], num, what);
            return BBGPU_ERR_ARG;
        }
    return BBGPU_OK;
}

int bbgpu_host_plonk_verify_multi(const bbgpu_plonk_verify_key* keys, int num_keys, const uint64_t g2_x[16], const uint32_t* circuit, const uint64_t* proofs,
                                  size_t count, const uint64_t seed[4], int flags, uint32_t* status, bbgpu_plonk_verify_report* out)
{
    if (int rc = verify_multi_args(keys, num_keys, "keys", circuit, proofs, count, flags, status, out)) return rc;
    std::vector<host::VerifyKey> K((size_t)num_keys);
    for (int c = 0; c < num_keys; c++) {
        const char* why = "";
        if (int rc = host::verify_key_init(&K[c], keys[c].n, keys[c].widgets, keys[c].vk, g2_x, &why)) {
            set_error("PLONK verify: key %d: %s", c, why);
            return rc;
        }
    }
    uint64_t sd[4];
    if (int rc = call_seed("PLONK verify", seed, sd)) return rc;
    return host::verify_host_multi(K.data(), K.size(), g2_x, circuit, proofs, count, sd, flags, status, out);
}

/* ---- SRS ---- */
int bbgpu_srs_register(const uint64_t* points_endo_table, size_t n)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    if (!points_endo_table || n == 0) return BBGPU_ERR_ARG;
    size_t off;
    int idx = find_srs(points_endo_table, n, &off);
    if (idx >= 0 && off == 0) {
        ctx().srs[idx].auto_registered = false; // the caller now holds the handle: never evicted behind its back
        ctx().srs[idx].handle_exposed = true;
        return idx;
    }
    uint32_t* d = nullptr;
    rc = srs_upload(points_endo_table, n, &d, ctx().stream);
    if (rc) return rc;
    return add_srs(points_endo_table, n, d, false);
}

int bbgpu_srs_generate_range(const uint64_t* x_mont, size_t first, size_t n, uint64_t* host_endo_table_out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int rc = ensure_init();
    if (rc) return rc;
    if (!x_mont || n == 0 || first > ((size_t)1 << 31) || n > ((size_t)1 << 31)) return BBGPU_ERR_ARG;
    uint32_t* d = nullptr;
    rc = srs_generate(x_mont, first, n, &d, host_endo_table_out, ctx().stream);
    if (rc) return rc;
    return add_srs(host_endo_table_out, n, d, false);
}
int bbgpu_srs_generate(const uint64_t* x_mont, size_t n, uint64_t* host_endo_table_out)
{
    return bbgpu_srs_generate_range(x_mont, 0, n, host_endo_table_out);
}

/* ---- the SRS update (host_srs_update.hpp, srs_update.hip) ---- */
static int srs_update_args(size_t n, size_t first_power, const uint64_t* y_mont, host::Fr* y)
{
    if (!y_mont || n == 0 || first_power > ((size_t)1 << 32) || n > ((size_t)1 << 32) - first_power) {
        set_error("SRS update: null y, n == 0 or first_power + n beyond 2^32");
        return BBGPU_ERR_ARG;
    }
    if (!host::srs_update_secret(y_mont, y)) {
        set_error("SRS update: y is zero modulo r");
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}

int bbgpu_host_srs_update(const uint64_t* points_endo_table, size_t n, size_t first_power, const uint64_t y_mont[4], const uint64_t g2_x[16],
                          uint64_t* table_out, bbgpu_srs_update_report* out)
{
    if (!points_endo_table || !table_out) {
        set_error("SRS update: null table");
        return BBGPU_ERR_ARG;
    }
    host::Fr y;
    if (int rc = srs_update_args(n, first_power, y_mont, &y)) return rc;
    bbgpu_srs_update_report rep;
    host::srs_update_report_init(&rep, n, first_power, y, g2_x);
    const int rc = host::srs_update_host(points_endo_table, n, first_power, y, table_out, &rep);
    if (out) *out = rep;
    if (rc) set_error("SRS update: row %llu is not on the curve (%llu such rows)", (unsigned long long)rep.first_bad_point, (unsigned long long)rep.bad_points);
    return rc;
}

int bbgpu_host_srs_update_check(const uint64_t old_p1[8], const uint64_t new_p1[8], const uint64_t y_g2[16], int* ok)
{
    if (!old_p1 || !new_p1 || !y_g2 || !ok) {
        set_error("null old_p1 / new_p1 / y_g2 / ok");
        return BBGPU_ERR_ARG;
    }
    *ok = host::srs_update_check(old_p1, new_p1, y_g2) ? 1 : 0;
    return BBGPU_OK;
}

int bbgpu_srs_update(int srs_handle, size_t n, size_t first_power, const uint64_t y_mont[4], const uint64_t g2_x[16], uint64_t* host_endo_table_out,
                     bbgpu_srs_update_report* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound: a handle can only exist once one is
    host::Fr y;
    if (int rc = srs_update_args(n, first_power, y_mont, &y)) return rc;
    const SrsEntry* ep = nullptr;
    if (int rc = srs_rows("SRS update", srs_handle, n, BBGPU_ERR_ARG, &ep)) return rc;
    if (int rc = ensure_init()) return rc;
    bbgpu_srs_update_report rep;
    host::srs_update_report_init(&rep, n, first_power, y, g2_x);
    const uint32_t* d_in = ep->d_srs; // add_srs below may move the registry: nothing of the entry is held across it
    const hipStream_t st = ctx().stream;
    if (int rc = curve_pass(d_in, n, 1, &rep.bad_points, &rep.first_bad_point)) return rc;
    if (out) *out = rep;
    if (rep.bad_points) {
        set_error("SRS update: row %llu is not on the curve (%llu such rows)", (unsigned long long)rep.first_bad_point, (unsigned long long)rep.bad_points);
        return BBGPU_ERR_ARG;
    }
    uint32_t* d = nullptr;
    float kernel_ms = 0;
    if (int rc = srs_update_rows(d_in, n, (uint64_t)first_power, y.d, &d, host_endo_table_out, st, ctx().timing ? &kernel_ms : nullptr)) return rc;
    if (ctx().timing) { // bbgpu_last_timing: index 0, the update kernel alone
        ctx().last.count = 1;
        ctx().last.ms[0] = kernel_ms;
    }
    return add_srs(host_endo_table_out, n, d, false);
}

/* ---- the SRS in the Lagrange basis (host_srs_lagrange.hpp, srs_lagrange.hip) ---- */
static int srs_lagrange_args(size_t n, int* log2n)
{
    if (n == 0) {
        set_error("SRS Lagrange basis: n == 0");
        return BBGPU_ERR_ARG;
    }
    if ((*log2n = host::srs_lagrange_log2(n)) < 0) {
        set_error("SRS Lagrange basis: n = %zu is not a power of two between 2 and 2^%d", n, host::SRS_LAGRANGE_MAX_LOG2);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}
static int srs_lagrange_refusal(const bbgpu_srs_lagrange_report& rep)
{
    if (rep.bad_points)
        set_error("SRS Lagrange basis: row %llu is not on the curve (%llu such rows)", (unsigned long long)rep.first_bad_point, (unsigned long long)rep.bad_points);
    else
        set_error("SRS Lagrange basis: output row %llu is the point at infinity (%llu such rows)", (unsigned long long)rep.first_infinity_row,
                  (unsigned long long)rep.infinity_rows);
    return BBGPU_ERR_ARG;
}

int bbgpu_host_srs_lagrange(const uint64_t* points_endo_table, size_t n, uint64_t* table_out, bbgpu_srs_lagrange_report* out)
{
    if (!points_endo_table || !table_out) {
        set_error("SRS Lagrange basis: null table");
        return BBGPU_ERR_ARG;
    }
    int log2n;
    if (int rc = srs_lagrange_args(n, &log2n)) return rc;
    bbgpu_srs_lagrange_report rep;
    host::srs_lagrange_report_init(&rep, n);
    const int rc = host::srs_lagrange_host(points_endo_table, n, log2n, table_out, &rep);
    if (out) *out = rep;
    return rc ? srs_lagrange_refusal(rep) : rc;
}

int bbgpu_srs_lagrange(int srs_handle, size_t n, uint64_t* host_endo_table_out, bbgpu_srs_lagrange_report* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound: a handle can only exist once one is
    int log2n;
    if (int rc = srs_lagrange_args(n, &log2n)) return rc;
    const SrsEntry* ep = nullptr;
    if (int rc = srs_rows("SRS Lagrange basis", srs_handle, n, BBGPU_ERR_SIZE, &ep)) return rc;
    if (int rc = ensure_init()) return rc;
    bbgpu_srs_lagrange_report rep;
    host::srs_lagrange_report_init(&rep, n);
    const uint32_t* d_in = ep->d_srs; // add_srs below may move the registry: nothing of the entry is held across it
    const hipStream_t st = ctx().stream;
    // two findings, started by the one upload: [0] the curve pass over the input rows, [1] the output rows at infinity
    if (int rc = curve_pass(d_in, n, 2, &rep.bad_points, &rep.first_bad_point)) return rc;
    SrsCurveFindings* d_find = reinterpret_cast<SrsCurveFindings*>(ctx().d_srs_check);
    SrsCurveFindings infinite = NO_FINDINGS;
    if (rep.bad_points) {
        if (out) *out = rep;
        return srs_lagrange_refusal(rep);
    }
    host::Fr winv, ninv;
    host::srs_lagrange_constants(log2n, &winv, &ninv);
    const Limbs9 wl = host::limbs_m261(winv);
    uint32_t* d = nullptr;
    float ms3[3] = { 0, 0, 0 };
    if (int rc = srs_lagrange_rows(d_in, n, log2n, wl.d, ninv.d, d_find + 1, &infinite, &d, host_endo_table_out, st, ctx().timing ? ms3 : nullptr)) return rc;
    rep.infinity_rows = infinite.bad_points;
    rep.first_infinity_row = infinite.bad_points ? infinite.first_bad_point : UINT64_MAX;
    if (out) *out = rep;
    if (ctx().timing) { // bbgpu_last_timing: index 0 the stage kernels alone, 1 the load (scaling) kernel, 2 the finish kernel
        ctx().last.count = 3;
        for (int i = 0; i < 3; i++) ctx().last.ms[i] = ms3[i];
    }
    if (rep.infinity_rows) return srs_lagrange_refusal(rep);
    return add_srs(host_endo_table_out, n, d, false);
}

/* ---- is this table the Lagrange form of that string?  (host_srs_lagrange_check.hpp; the parts of bbgpu_srs_check, no kernel of its own) ---- */
static int srs_lagrange_check_args(size_t n, int flags, const void* out, int* log2n)
{
    if (!out || (flags & ~BBGPU_SRS_LAGRANGE_CHECK_LOCATE)) {
        set_error("SRS Lagrange check: null out or unknown flag bits 0x%x", flags);
        return BBGPU_ERR_ARG;
    }
    if ((*log2n = host::srs_lagrange_log2(n)) < 0) {
        set_error("SRS Lagrange check: n = %zu is not a power of two between 2 and 2^%d", n, host::SRS_LAGRANGE_MAX_LOG2);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}

int bbgpu_host_srs_lagrange_check(const uint64_t* lagrange_endo_table, const uint64_t* monomial_endo_table, size_t n, const uint64_t seed[4], int flags,
                                  bbgpu_srs_lagrange_check_report* out)
{
    if (!lagrange_endo_table || !monomial_endo_table) {
        set_error("SRS Lagrange check: null table");
        return BBGPU_ERR_ARG;
    }
    int log2n;
    if (int rc = srs_lagrange_check_args(n, flags, out, &log2n)) return rc;
    uint64_t sd[4];
    if (int rc = call_seed("SRS Lagrange check", seed, sd)) return rc;
    return host::srs_lagrange_check_host(lagrange_endo_table, monomial_endo_table, n, log2n, sd, flags, out);
}

int bbgpu_srs_lagrange_check(int lagrange_handle, int monomial_handle, size_t n, const uint64_t seed[4], int flags, bbgpu_srs_lagrange_check_report* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound: a handle can only exist once one is
    int log2n;
    if (int rc = srs_lagrange_check_args(n, flags, out, &log2n)) return rc;
    const SrsEntry *el = nullptr, *em = nullptr;
    if (int rc = srs_rows("SRS Lagrange check", lagrange_handle, n, BBGPU_ERR_SIZE, &el, true)) return rc;
    if (int rc = srs_rows("SRS Lagrange check", monomial_handle, n, BBGPU_ERR_SIZE, &em, true)) return rc;
    if (int rc = ensure_init()) return rc;
    uint64_t sd[4];
    if (int rc = call_seed("SRS Lagrange check", seed, sd)) return rc;
    host::srs_lagrange_check_report_init(out, n, sd);
    // behind the findings: the n multipliers, made beside the curve pass, and the copy of them that is transformed
    uint64_t* d_rho = nullptr;
    if (int rc = curve_pass(el->d_srs, n, nullptr, 2 * n * 32, 1, [&](uint64_t* d_extra, hipStream_t st) { return srs_check_scalars(sd, n, d_rho = d_extra, st); },
                            &out->bad_points, &out->first_bad_point))
        return rc;
    if (out->bad_points) return BBGPU_OK;
    uint64_t* d_coef = d_rho + 4 * n;
    const hipStream_t st = ctx().stream;
    // A and B: the copy is cut and transformed on the library's stream, then two tickets in flight
    return host::srs_lagrange_check_basis(out, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) -> int {
        HIPCHK(hipMemcpyAsync(d_coef, d_rho, m * 32, hipMemcpyDeviceToDevice, st));
        if (m < n) HIPCHK(hipMemsetAsync(d_coef + 4 * m, 0, (n - m) * 32, st));
        if (int rc = bbgpu_ntt_device(d_coef, n, BBGPU_IFFT, nullptr, st)) return rc;
        HIPCHK(hipStreamSynchronize(st)); // the tickets run on slot streams
        return two_msms(*el, 0, d_rho, m, *em, 0, d_coef, n, a12, b12);
    });
}

// io.hpp:36-182 restated for the G1 part: 28-byte manifest of seven big-endian uint32 (fields 5 = num_g1_points), then points as
// x, y, each four 64-bit limbs least-significant limb first, every limb big-endian, NOT in Montgomery form; file point k is
// x^(k+1) G and monomials[0] is the generator (read_transcript :159-181).  Fills the complete 2n-entry endomorphism table of
// generate_pippenger_point_table (scalar_multiplication.cpp:131-140): entry 2i = P_i, entry 2i+1 = (beta x_i, -y_i).  Host only.
/* ---- a polynomial opened at every point of its domain (all n KZG proofs at once) or on every coset of it (all n / l cell proofs): one host twin and one
 * device path, kzg_open_cosets.hip, for both families of entries -- open-all is the coset size 1 without a bound (host_kzg_open_all.hpp,
 * host_kzg_open_cosets.hpp).  What differs between the families is the pool of setups and the wording of the verdicts on n ---- */
static int open_all_n(const char* what, size_t n, int* log2n)
{
    if ((*log2n = host::kzg_open_all_log2(n)) < 0) {
        set_error("%s: n = %zu is not a power of two between 2 and 2^%d", what, n, host::KZG_OPEN_ALL_MAX_LOG2);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}
static int open_all_batch(const char* what, int batch)
{
    if (batch < 1 || batch > host::KZG_OPEN_ALL_MAX_BATCH) {
        set_error("%s: batch = %d must be in 1..%d", what, batch, host::KZG_OPEN_ALL_MAX_BATCH);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}
static int open_cosets_n(const char* what, size_t n, size_t coset, int* log2n, int* log2l)
{
    if (!host::kzg_open_cosets_log2(n, coset, log2n, log2l)) {
        set_error("%s: n = %zu must be a power of two between 2 and 2^%d and the coset size (%zu) a power of two between 1 and %d, at most n / 2", what, n,
                  host::KZG_OPEN_ALL_MAX_LOG2, coset, BBGPU_KZG_OPEN_COSETS_MAX_COSET);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}
// the degree bound of a setup of (n, l)
static int open_cosets_bound(const char* what, int log2n, int log2l, size_t degree_bound, int* log2d)
{
    if ((*log2d = host::kzg_open_cosets_bound_log2(log2n, log2l, degree_bound)) < 0) {
        set_error("%s: the degree bound (%zu) must be a power of two between twice the coset size (%zu) and n = %zu", what, degree_bound, (size_t)2 << log2l,
                  (size_t)1 << log2n);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}
// the sizes of one call over a setup of (n, d); d == n, as of every open-all setup, speaks of n alone
static int open_cosets_sizes(const char* what, size_t n, size_t d, size_t stride_elems, int batch)
{
    if (!host::kzg_open_cosets_sizes_ok(n, d, stride_elems, batch)) {
        set_error("%s: the stride (%zu) must be no smaller than %s = %zu and batch x 2 n (%d x %zu) at most 2^%d", what, stride_elems,
                  d == n ? "n" : "the degree bound", d, batch, 2 * n, host::KZG_OPEN_ALL_MAX_SLOTS_LOG2);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}
// (n, l, d) of an entry of either family.  cosets == false: an open-all entry, which knows of no coset size and no bound -- n alone is judged, in
// open_all_n's words, and l = 1, d = n
static int open_shape(const char* what, bool cosets, size_t n, size_t coset, size_t degree_bound, int* log2n, int* log2l, int* log2d)
{
    if (!cosets) {
        *log2l = 0;
        const int rc = open_all_n(what, n, log2n);
        *log2d = *log2n;
        return rc;
    }
    if (int rc = open_cosets_n(what, n, coset, log2n, log2l)) return rc;
    return open_cosets_bound(what, *log2n, *log2l, degree_bound, log2d);
}

// the host twin of either family (open-all: coset = 1, degree_bound = n)
static int open_host(const char* what, bool cosets, const uint64_t* points_endo_table, size_t n, size_t coset, size_t degree_bound, const uint64_t* coeffs,
                     size_t stride_elems, int batch, uint64_t* proofs_out)
{
    int log2n, log2l, log2d;
    if (int rc = open_shape(what, cosets, n, coset, degree_bound, &log2n, &log2l, &log2d)) return rc;
    if (int rc = open_all_batch(what, batch)) return rc;
    if (!points_endo_table || !coeffs || !proofs_out) {
        set_error("%s: null table / coeffs / proofs", what);
        return BBGPU_ERR_ARG;
    }
    if (int rc = open_cosets_sizes(what, n, degree_bound, stride_elems, batch)) return rc;
    std::vector<host::Xyzz> S;
    uint64_t bad = 0;
    if (host::kzg_open_cosets_setup_bounded_host(points_endo_table, log2d, log2l, S, &bad)) {
        set_error("%s: row %llu is not on the curve", what, (unsigned long long)bad);
        return BBGPU_ERR_ARG;
    }
    host::kzg_open_cosets_proofs_bounded_host(S, log2n, log2l, log2d, coeffs, stride_elems, batch, proofs_out);
    return BBGPU_OK;
}

// a setup in `pool` (open-all: coset = 1, degree_bound = n) -> its handle, the lowest free slot of that pool
static int open_setup_make(OpenPool& pool, const char* what, bool cosets, int srs_handle, size_t n, size_t coset, size_t degree_bound)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound: a handle can only exist once one is
    int log2n, log2l, log2d;
    if (int rc = open_shape(what, cosets, n, coset, degree_bound, &log2n, &log2l, &log2d)) return rc;
    const SrsEntry* ep = nullptr;
    if (int rc = srs_rows(what, srs_handle, degree_bound, BBGPU_ERR_SIZE, &ep)) return rc; // d rows serve every n
    int slot = -1;
    for (int k = 0; k < OPEN_MAX_SETUPS && slot < 0; k++)
        if (!pool[k].live) slot = k;
    if (slot < 0) {
        set_error("%s: %d setups are live", what, OPEN_MAX_SETUPS);
        return BBGPU_ERR_STATE;
    }
    if (int rc = ensure_init()) return rc;
    const uint32_t* d_in = ep->d_srs;
    const hipStream_t st = ctx().stream;
    // the curve pass over the rows the strings read, [0, d - l)
    uint64_t bad_points, first_bad_point;
    if (int rc = curve_pass(d_in, degree_bound - coset, 1, &bad_points, &first_bad_point)) return rc;
    if (bad_points) {
        set_error("%s: row %llu is not on the curve (%llu such rows)", what, (unsigned long long)first_bad_point, (unsigned long long)bad_points);
        return BBGPU_ERR_ARG;
    }
    const Limbs9 W = host::limbs_m261(host::fr_root_of_unity(log2d - log2l + 1));
    OpenSetup o;
    if (int rc = kzg_open_cosets_string(d_in, log2d, log2l, W.d, &o.d_S, st)) return rc;
    o.log2n = log2n;
    o.log2l = log2l;
    o.log2d = log2d;
    o.bytes = 2 * degree_bound * 128;
    o.live = true;
    pool[slot] = o;
    return slot;
}

static int open_setup_release(OpenPool& pool, const char* what, int setup)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (setup < 0 || setup >= OPEN_MAX_SETUPS || !pool[setup].live) {
        set_error("%s: unknown setup %d", what, setup);
        return BBGPU_ERR_ARG;
    }
    open_release(pool[setup]); // (dev_free waits for the device: no queued call still reads S^)
    return BBGPU_OK;
}

// one call over a setup of `pool`
static int open_call(const OpenPool& pool, const char* what, int setup, const uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* proofs_out,
                     void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (int rc = open_all_batch(what, batch)) return rc;
    if (!d_coeffs || !proofs_out) {
        set_error("%s: null coeffs / proofs", what);
        return BBGPU_ERR_ARG;
    }
    if (setup < 0 || setup >= OPEN_MAX_SETUPS || !pool[setup].live) {
        set_error("%s: unknown setup %d", what, setup);
        return BBGPU_ERR_ARG;
    }
    const OpenSetup& o = pool[setup];
    const int log2M = o.log2d - o.log2l + 1; // M = 2 mu = 2 d / l
    const size_t n = (size_t)1 << o.log2n, d = (size_t)1 << o.log2d, l = (size_t)1 << o.log2l, m = n >> o.log2l, M = (size_t)1 << log2M;
    if (int rc = open_cosets_sizes(what, n, d, stride_elems, batch)) return rc;
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    // t, then t^, then the proofs: batch x 2 d x 32 bytes of scalars, batch x m x 64 of proofs -- the larger of the two (the scalars unless d < m; at d = n
    // they hold the proofs l times over); and the 2 m scratch points of every polynomial: the convolution in [0, M), the forward transform in [m, 2 m)
    DevBuf t, scratch;
    HIPCHK(dev_malloc(&t.p, (size_t)batch * std::max(2 * d * 32, m * 64)));
    HIPCHK(dev_malloc(&scratch.p, (size_t)batch * 2 * m * 128));
    if (int rc = kzg_open_cosets_t(d_coeffs, stride_elems, batch, o.log2d, o.log2l, t.as<uint64_t>(), st)) return rc;
    // batch x l transforms of length M, side by side; the batched transform takes KZG_OPEN_ALL_MAX_BATCH of them per call (one call at l = 1)
    for (size_t done = 0, all = (size_t)batch * l; done < all; done += host::KZG_OPEN_ALL_MAX_BATCH) {
        const int group = (int)std::min<size_t>(all - done, host::KZG_OPEN_ALL_MAX_BATCH);
        if (int rc = bbgpu_ntt_device_batch(t.as<uint64_t>() + done * M * 4, M, M, group, BBGPU_FFT, nullptr, hip_stream)) return rc;
    }
    const host::Fr W = host::fr_root_of_unity(log2M);
    const host::Fr c32 = host::fr_from_mont(host::fr_mul(host::fr_inv(host::fr_from_u64((uint64_t)M)), host::fr_from_u64(32))); // the plain integer 32 / M
    float ms4[4] = { 0, 0, 0, 0 };
    if (int rc = kzg_open_cosets_chain(o.d_S, t.as<uint64_t>(), scratch.as<uint32_t>(), o.log2n, o.log2l, o.log2d, batch, host::limbs_m256(c32).d,
                                       host::limbs_m261(host::fr_inv(W)).d, host::limbs_m261(host::fr_root_of_unity(o.log2n - o.log2l)).d, st,
                                       ctx().timing ? ms4 : nullptr))
        return rc;
    if (int rc = device_to_host_sync(proofs_out, t.p, (size_t)batch * m * 64, st)) return rc;
    if (ctx().timing) { // bbgpu_last_timing: index 0 the sum kernel, 1 the inverse stages, 2 the gather kernel and the forward stages, 3 the finish kernel
        ctx().last.count = 4;
        for (int i = 0; i < 4; i++) ctx().last.ms[i] = ms4[i];
    }
    return BBGPU_OK;
}

int bbgpu_host_kzg_open_all(const uint64_t* points_endo_table, size_t n, const uint64_t* coeffs, size_t stride_elems, int batch, uint64_t* proofs_out)
{
    return open_host("host kzg_open_all", false, points_endo_table, n, 1, n, coeffs, stride_elems, batch, proofs_out);
}
int bbgpu_kzg_open_all_setup(int srs_handle, size_t n) { return open_setup_make(g_open_all, "kzg_open_all_setup", false, srs_handle, n, 1, n); }
int bbgpu_kzg_open_all_release(int setup) { return open_setup_release(g_open_all, "kzg_open_all_release", setup); }
int bbgpu_kzg_open_all_device(int setup, const uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* proofs_out, void* hip_stream)
{
    return open_call(g_open_all, "kzg_open_all", setup, d_coeffs, stride_elems, batch, proofs_out, hip_stream);
}

int bbgpu_host_kzg_open_cosets_bounded(const uint64_t* points_endo_table, size_t n, size_t coset, size_t degree_bound, const uint64_t* coeffs, size_t stride_elems,
                                       int batch, uint64_t* proofs_out)
{
    return open_host("host kzg_open_cosets", true, points_endo_table, n, coset, degree_bound, coeffs, stride_elems, batch, proofs_out);
}
int bbgpu_host_kzg_open_cosets(const uint64_t* points_endo_table, size_t n, size_t coset, const uint64_t* coeffs, size_t stride_elems, int batch,
                               uint64_t* proofs_out)
{
    int log2n, log2l;
    if (int rc = open_cosets_n("host kzg_open_cosets", n, coset, &log2n, &log2l)) return rc; // (the bound of the call below is n: never refused)
    return bbgpu_host_kzg_open_cosets_bounded(points_endo_table, n, coset, n, coeffs, stride_elems, batch, proofs_out);
}
int bbgpu_kzg_open_cosets_setup_bounded(int srs_handle, size_t n, size_t coset, size_t degree_bound)
{
    return open_setup_make(g_open_cosets, "kzg_open_cosets_setup", true, srs_handle, n, coset, degree_bound);
}
int bbgpu_kzg_open_cosets_setup(int srs_handle, size_t n, size_t coset) { return bbgpu_kzg_open_cosets_setup_bounded(srs_handle, n, coset, n); }
int bbgpu_kzg_open_cosets_release(int setup) { return open_setup_release(g_open_cosets, "kzg_open_cosets_release", setup); }
int bbgpu_kzg_open_cosets_device(int setup, const uint64_t* d_coeffs, size_t stride_elems, int batch, uint64_t* proofs_out, void* hip_stream)
{
    return open_call(g_open_cosets, "kzg_open_cosets", setup, d_coeffs, stride_elems, batch, proofs_out, hip_stream);
}

int bbgpu_transcript_read_g1(const char* path, size_t degree, uint64_t* points_endo_table_out)
{
    if (!path || !points_endo_table_out || degree == 0) return BBGPU_ERR_ARG;
    FILE* f = fopen(path, "rb");
    if (!f) {
        set_error("cannot open transcript %s", path);
        return BBGPU_ERR_ARG;
    }
    unsigned char man[28];
    if (fread(man, 1, 28, f) != 28) {
        fclose(f);
        set_error("transcript %s: short manifest", path);
        return BBGPU_ERR_SIZE;
    }
    auto be32 = [&](int i) { return ((uint32_t)man[4 * i] << 24) | ((uint32_t)man[4 * i + 1] << 16) | ((uint32_t)man[4 * i + 2] << 8) | man[4 * i + 3]; };
    const uint32_t num_g1 = be32(4);
    if ((size_t)num_g1 + 1 < degree) {
        fclose(f);
        set_error("transcript %s holds %u G1 points, %zu needed", path, num_g1, degree - 1);
        return BBGPU_ERR_SIZE;
    }
    const host::Fq rsq = { { 0xF32CFC5B538AFA89ULL, 0xB5E71911D44501FBULL, 0x47AB1EFF0A417FF6ULL, 0x06D89F71CAB8351FULL } }; // 2^512 mod q (fq.hpp:48-51)
    const host::Fq beta = { { 0x71930c11d782e155ULL, 0xa6bb947cffbe3323ULL, 0xaa303344d4741444ULL, 0x2c3b3f0d26594943ULL } }; // fq.hpp:53-56 (Montgomery)
    const host::Fq zero = { { 0, 0, 0, 0 } };
    auto put = [&](size_t i, const host::Fq& x, const host::Fq& y) {
        uint64_t* e = points_endo_table_out + i * 16;
        memcpy(e, x.d, 32);
        memcpy(e + 4, y.d, 32);
        const host::Fq bx = host::fq_mul(x, beta), ny = host::fq_sub(zero, y);
        memcpy(e + 8, bx.d, 32);
        memcpy(e + 12, ny.d, 32);
    };
    host::Fq two = host::fq_add(host::FQ_ONE, host::FQ_ONE);
    put(0, host::FQ_ONE, two); // g1::affine_one = (1, 2) (g1.hpp:14-16)
    std::vector<unsigned char> buf(64 * 4096);
    size_t done = 1;
    while (done < degree) {
        const size_t chunk = std::min<size_t>(4096, degree - done);
        if (fread(buf.data(), 64, chunk, f) != chunk) {
            fclose(f);
            set_error("transcript %s: short read", path);
            return BBGPU_ERR_SIZE;
        }
        for (size_t k = 0; k < chunk; k++) {
            host::Fq c[2];
            for (int xy = 0; xy < 2; xy++)
                for (int l = 0; l < 4; l++) {
                    uint64_t v = 0;
                    for (int b = 0; b < 8; b++) v = (v << 8) | buf[k * 64 + xy * 32 + l * 8 + b];
                    c[xy].d[l] = v;
                }
            put(done + k, host::fq_mul(c[0], rsq), host::fq_mul(c[1], rsq));
        }
        done += chunk;
    }
    fclose(f);
    return BBGPU_OK;
}

// io.hpp:36-135,159-181 restated for WRITING: the file read_transcript(monomials, g2_x, degree, path) accepts for this SRS.
// 28-byte manifest (seven big-endian uint32: transcript_number 0, total_transcripts 1, total_g1_points, total_g2_points 2, num_g1_points,
// num_g2_points 2, start_from 0), the degree - 1 points x G .. x^(degree-1) G (entries 2 .. 2 (degree - 1) of the endo table; entry 0, the
// generator, is implicit in the format), then G2 and x G2, then the 64-byte checksum slot the reference never verifies (zeros).
// Coordinates leave Montgomery form; four 64-bit limbs least-significant first, each limb big-endian.  Host only.
int bbgpu_transcript_write(const char* path, const uint64_t* points_endo_table, size_t degree, const uint64_t x_mont[4])
{
    if (!path || !points_endo_table || degree < 2 || !x_mont || degree - 1 > 0xffffffffu) return BBGPU_ERR_ARG;
    host::G2Affine xg2;
    if (!host::g2_scalar_mul_affine(host::G2_ONE, load_fr(x_mont), &xg2)) {
        set_error("transcript secret is zero");
        return BBGPU_ERR_ARG;
    }
    const char* why = "";
    if (!host::transcript_write_file(path, points_endo_table, degree, xg2, &why)) {
        set_error("%s %s", why, path);
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}

// the same file for a string whose secret nobody holds (an updated one): x G2 is the caller's, checked as bbgpu_srs_check checks it.  Host only.
int bbgpu_transcript_write_g2(const char* path, const uint64_t* points_endo_table, size_t degree, const uint64_t g2_x[16])
{
    if (!path || !points_endo_table || degree < 2 || !g2_x || degree - 1 > 0xffffffffu) {
        set_error("transcript: null path / table / g2_x, degree < 2 or beyond 2^32");
        return BBGPU_ERR_ARG;
    }
    if (!host::srs_check_g2_ok(g2_x)) {
        set_error("transcript x * G2 is not a point of G2");
        return BBGPU_ERR_ARG;
    }
    const char* why = "";
    if (!host::transcript_write_file(path, points_endo_table, degree, host::g2_from_words(g2_x), &why)) {
        set_error("%s %s", why, path);
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}

int bbgpu_srs_set_validate(int srs_handle, int full)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (srs_handle == -1) {
        for (auto& C : g_ctxs) C.srs_validate_full = full != 0;
        return BBGPU_OK;
    }
    if (srs_handle < 0 || srs_handle >= (int)ctx().srs.size() || !ctx().srs[srs_handle].live) return BBGPU_ERR_ARG;
    ctx().srs[srs_handle].validate_full = full != 0;
    return BBGPU_OK;
}

int bbgpu_srs_release(int handle)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (handle < 0 || handle >= (int)ctx().srs.size() || !ctx().srs[handle].live) return BBGPU_ERR_ARG;
    free_entry(ctx().srs[handle]);
    return BBGPU_OK;
}

// resident tables right now: how many, how many of them registered on first sight (evictable), device bytes held by those
int bbgpu_srs_cache_stats(int* live_entries, int* auto_entries, uint64_t* auto_bytes)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    int live = 0, au = 0;
    uint64_t bytes = 0;
    for (const auto& e : ctx().srs)
        if (e.live) {
            live++;
            if (e.auto_registered) {
                au++;
                bytes += e.bytes;
            }
        }
    if (live_entries) *live_entries = live;
    if (auto_entries) *auto_entries = au;
    if (auto_bytes) *auto_bytes = bytes;
    return BBGPU_OK;
}

/* ---- MSM ---- */
int bbgpu_msm_num_windows(size_t n)
{
    return msm_num_windows(msm_choose_c(n ? n : 1));
}
int bbgpu_srs_num_windows(int srs_handle, size_t n)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (srs_handle < 0 || srs_handle >= (int)ctx().srs.size() || !ctx().srs[srs_handle].live) return BBGPU_ERR_ARG;
    return entry_windows(ctx().srs[srs_handle], n);
}
// Multi-GPU: rank `rank` of `world` will only ever be asked for its 1/world share of the (window, point) rows of tables registered
// from now on, so only the digit windows that share touches are built and kept: 15 x 64 MiB at n = 2^20 become ceil(15 / world) + 1 windows.
void bbgpu_set_table_share(int rank, int world)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (world < 1 || rank < 0 || rank >= world) { rank = 0; world = 1; }
    ctx().share_rank = rank;
    ctx().share_world = world;
}

// Multi-GPU, the other split: a rank holds n / world POINTS of a larger MSM as its own SRS (all digit windows of them) and its MSM over the matching
// scalars is its partial sum.  Tables registered from now on pick their window size as the whole MSM would.
void bbgpu_set_point_share(int world)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    ctx().point_world = world >= 1 && world <= 1024 ? world : 1;
}

void bbgpu_set_precompute(int enabled)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    for (auto& C : g_ctxs) C.precompute = enabled != 0;
}

int bbgpu_msm_g1(const uint64_t* scalars, const uint64_t* points_endo_table, size_t n, uint64_t out[12])
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    multi::Slice sl[BBGPU_MAX_CONTEXTS];
    const int m = multi::plan_slices(n, g_num_ctx, sl);
    if (m == 1) return msm_host_ptrs(scalars, points_endo_table, n, out); // binds the device itself unless the host answers (n = 0, tiny unknown tables)
    if (!scalars || !points_endo_table) {
        set_error("null scalars/points");
        return BBGPU_ERR_ARG;
    }
    // context k: points [first, first + len) with their own cache lookup / registration on first sight, exact-mode rerun and two-range pipeline
    host::Xyzz part[BBGPU_MAX_CONTEXTS];
    const int rc = run_on_contexts(m, [&](int k) {
        ctx().slice_of_n = n;
        const int r = msm_host_ptrs_sum(scalars + 4 * sl[k].first, points_endo_table + 16 * sl[k].first, sl[k].len, &part[k]);
        ctx().slice_of_n = 0;
        return r;
    });
    if (rc) return rc;
    host::Xyzz acc = part[0];
    for (int k = 1; k < m; k++) acc = host::g1_add(acc, part[k]); // equal partial sums double, opposite ones cancel (host_g1.hpp)
    host::g1_to_normalised(acc, out);
    return BBGPU_OK;
}

int bbgpu_msm_g1_plain(const uint64_t* scalars, const uint64_t* points, size_t n, uint64_t out[12])
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return msm_host_ptrs(scalars, points, n, out, true);
}

void bbgpu_set_host_thresholds(int msm_max_points, int ntt_max_elements)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    for (auto& C : g_ctxs) {
        C.host_env_read = true;
        C.host_msm_max = msm_max_points < 0 ? 0 : msm_max_points;
        C.host_ntt_max = ntt_max_elements < 0 ? 0 : std::min(64, ntt_max_elements);
    }
}

// scalar_multiplication.cpp:678-685: report and leave the outputs untouched
static int batch_equal_sizes(const bbgpu_msm_job* jobs, size_t num_jobs)
{
    for (size_t i = 1; i < num_jobs; i++)
        if (jobs[i].num_elements != jobs[0].num_elements) {
            set_error("batched_scalar_multiplications err: each scalar mul must be same size.");
            return BBGPU_ERR_ARG;
        }
    return BBGPU_OK;
}
// tiny jobs go one at a time through msm_host_ptrs*: the host may answer them (caller has called read_host_env())
static bool batch_job_by_job(size_t n) { return n == 0 || n <= (size_t)ctx().host_msm_max; }
// Job i of a batch of n-point jobs has a null pointer while `slots` MSM slots are free.  done: how many jobs have their outputs written by then -- job by
// job every earlier one; through the pipeline those collected when room is made for job i's first range (what two slots leave in flight is one
// range, the last of job i-1).  numbered: the text names the job, which it does only where two slots run the pipeline, as it always has
struct NullJob { size_t done; bool numbered; };
static NullJob batch_null_job(size_t n, size_t i, int slots)
{
    if (batch_job_by_job(n)) return NullJob{ i, false };
    return NullJob{ collected_before(i, slots), slots >= 2 };
}
static int null_job_error(const NullJob& nj, size_t i)
{
    set_error(nj.numbered ? "null scalars/points in job %zu" : "null scalars/points", i);
    return BBGPU_ERR_ARG;
}
static int msm_g1_batch_once(bbgpu_msm_job* jobs, size_t num_jobs, bool* stale, host::Xyzz* sums);
// sums: null -- each job's normalised result goes to its output; else job i's sum goes to sums[i], not normalised (a context's partial sums of a split batch)
static int msm_g1_batch_run(bbgpu_msm_job* jobs, size_t num_jobs, host::Xyzz* sums)
{
    return rerun_if_stale([&](bool* stale) { return msm_g1_batch_once(jobs, num_jobs, stale, sums); });
}
// the first num_jobs jobs of a batch of equal sizes, non-null pointers, split over m contexts (slices sl): context k takes its slice of EVERY job
// through its own slot pipeline (as the reference's threads each take a range of every job, :703-738); each job's output is the fold of its
// m partial sums
static int msm_g1_batch_split(bbgpu_msm_job* jobs, size_t num_jobs, const multi::Slice* sl, int m)
{
    if (num_jobs == 0) return BBGPU_OK;
    const size_t n = jobs[0].num_elements;
    std::vector<bbgpu_msm_job> local((size_t)m * num_jobs);
    std::vector<host::Xyzz> part((size_t)m * num_jobs);
    for (int k = 0; k < m; k++)
        for (size_t i = 0; i < num_jobs; i++) {
            bbgpu_msm_job& J = local[(size_t)k * num_jobs + i];
            J = jobs[i];
            J.points = jobs[i].points + 16 * sl[k].first;
            J.scalars = jobs[i].scalars + 4 * sl[k].first;
            J.num_elements = sl[k].len;
        }
    const int rc = run_on_contexts(m, [&](int k) {
        ctx().slice_of_n = n;
        const int r = msm_g1_batch_run(&local[(size_t)k * num_jobs], num_jobs, &part[(size_t)k * num_jobs]);
        ctx().slice_of_n = 0;
        return r;
    });
    if (rc) return rc;
    for (size_t i = 0; i < num_jobs; i++) {
        host::Xyzz acc = part[i];
        for (int k = 1; k < m; k++) acc = host::g1_add(acc, part[(size_t)k * num_jobs + i]);
        host::g1_to_normalised(acc, jobs[i].output);
    }
    return BBGPU_OK;
}
int bbgpu_msm_g1_batch(bbgpu_msm_job* jobs, size_t num_jobs)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    multi::Slice sl[BBGPU_MAX_CONTEXTS];
    const int m = (num_jobs && jobs) ? multi::plan_slices(jobs[0].num_elements, g_num_ctx, sl) : 1;
    if (m == 1) return msm_g1_batch_run(jobs, num_jobs, nullptr);
    // split over the contexts.  The checks of msm_g1_batch_once come first, on the caller's thread, with what one context does on them: unequal sizes
    // leave every output untouched; a null job i ends the batch with the outputs of the jobs one context would have finished by then written
    if (int rc = batch_equal_sizes(jobs, num_jobs)) return rc;
    const size_t n = jobs[0].num_elements;
    for (size_t i = 0; i < num_jobs; i++)
        if (!jobs[i].scalars || !jobs[i].points) {
            read_host_env();
            int fs[2];
            const NullJob nj = batch_null_job(n, i, free_slots(fs, 2));
            if (int rc = msm_g1_batch_split(jobs, nj.done, sl, m)) return rc;
            return null_job_error(nj, i);
        }
    return msm_g1_batch_split(jobs, num_jobs, sl, m);
}
static int msm_g1_batch_once(bbgpu_msm_job* jobs, size_t num_jobs, bool* stale, host::Xyzz* sums)
{
    *stale = false;
    int rc = BBGPU_OK;
    if (num_jobs == 0) return BBGPU_OK;
    if (!jobs) return BBGPU_ERR_ARG;
    if ((rc = batch_equal_sizes(jobs, num_jobs)) != BBGPU_OK) return rc;
    const size_t n = jobs[0].num_elements;
    read_host_env();
    if (batch_job_by_job(n)) {
        for (size_t i = 0; i < num_jobs; i++) {
            rc = sums ? msm_host_ptrs_sum(jobs[i].scalars, jobs[i].points, jobs[i].num_elements, &sums[i])
                      : msm_host_ptrs(jobs[i].scalars, jobs[i].points, jobs[i].num_elements, jobs[i].output);
            if (rc) return rc;
        }
        return BBGPU_OK;
    }
    // The jobs go through the slot pipeline one range each -- a job above one table segment one range per segment it touches, like any other.  The tag
    // of a range is its job, with the low bit set on the job's last range: ranges are collected in issue order, so one running sum serves
    auto null_job = [&](size_t i) { return !jobs[i].scalars || !jobs[i].points; };
    int fs[2]; // job 0's pointers come before the slots it would need, as a single call's do: with none free it is still the null job that is reported
    if (null_job(0)) return null_job_error(batch_null_job(n, 0, free_slots(fs, 2)), 0);
    host::Xyzz acc = host::g1_infinity();
    HostMsmPipeline P([&](size_t tag, const host::Xyzz& part) {
        acc = host::g1_add(acc, part);
        if (!(tag & 1)) return;
        if (sums) sums[tag >> 1] = acc;
        else host::g1_to_normalised(acc, jobs[tag >> 1].output);
        acc = host::g1_infinity();
    });
    if ((rc = P.open()) != BBGPU_OK) return rc;
    const bool tr = trace_srs();
    for (size_t i = 0; i < num_jobs; i++) {
        const double push0 = P.ms_push, wait0 = P.ms_wait;
        if ((rc = P.make_room()) != BBGPU_OK) return rc; // before the job is looked at: what a null job leaves written does not depend on the job
        if (null_job(i)) return null_job_error(batch_null_job(n, i, P.ns), i);
        const double q1 = tr ? now_ms() : 0;
        size_t off = 0;
        bool full_check = false;
        int idx = find_srs(jobs[i].points, n, &off, &full_check);
        if (idx < 0) {
            uint32_t* d = nullptr;
            if ((rc = srs_upload(jobs[i].points, n, &d, ctx().stream)) != BBGPU_OK) return rc;
            if ((idx = add_srs(jobs[i].points, n, d, true)) < 0) return idx;
        }
        if (full_check) P.check_in_full(idx, off, jobs[i].points, n, false);
        const double q2 = tr ? now_ms() : 0;
        PointPiece pc[MAX_POINT_PIECES];
        const int np = split_pieces(ctx().srs[idx], off, n, pc, MAX_POINT_PIECES);
        if (np < 0) return BBGPU_ERR_SIZE;
        const size_t stage_bytes = largest_piece(pc, np) * 32;
        for (int k = 0; k < np; k++)
            if ((rc = P.push(ctx().srs[idx], off + pc[k].first, jobs[i].scalars + pc[k].first * 4, pc[k].len, stage_bytes, i * 2 + (k + 1 == np), nullptr)) != BBGPU_OK) return rc;
        if (tr) fprintf(stderr, "bbgpu batch: job %zu (%d ranges) srs %.3f, upload + issue %.3f, wait for earlier jobs %.3f ms\n", i, np, q2 - q1, P.ms_push - push0, P.ms_wait - wait0);
    }
    const double wait0 = P.ms_wait;
    rc = P.finish(stale);
    if (tr) fprintf(stderr, "bbgpu batch: last wait %.3f ms\n", P.ms_wait - wait0);
    return rc;
}

// what the two share entries check before they take a slot (kind: "row" / "bucket")
static int share_ticket_srs(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, const char* kind, const SrsEntry** ep)
{
    if (int rc = ticket_srs(srs_handle, ep)) return rc;
    const SrsEntry& e = **ep;
    if (offset + n > e.n || !d_scalars || n == 0) {
        set_error("MSM range [%zu, %zu) outside the registered table of %zu points", offset, offset + n, e.n);
        return BBGPU_ERR_ARG;
    }
    if (e.segs.size() != 1) {
        set_error(e.has_tab() ? "%s-range shares need ONE table segment: this SRS of %zu points keeps %zu (split it by point range instead)"
                              : "%s-range shares need the pre-shifted window tables (one shared bucket set): this table has none", kind, e.n, e.segs.size());
        return BBGPU_ERR_STATE;
    }
    return BBGPU_OK;
}
int bbgpu_msm_g1_device(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, int window_begin, int window_end,
                        uint64_t out[12], void* hip_stream)
{
    int ticket = bbgpu_msm_g1_device_async(srs_handle, offset, d_scalars, n, window_begin, window_end, hip_stream);
    if (ticket < 0) return ticket;
    return bbgpu_msm_g1_wait(ticket, out);
}

int bbgpu_msm_g1_device_async(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, int window_begin, int window_end,
                              void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const SrsEntry* ep = nullptr;
    if (int rc = ticket_srs(srs_handle, &ep)) return rc;
    const SrsEntry& e = *ep;
    if (offset + n > e.n || (!d_scalars && n)) {
        set_error("MSM range [%zu, %zu) outside the registered table of %zu points", offset, offset + n, e.n);
        return BBGPU_ERR_ARG;
    }
    int t;
    hipStream_t st;
    if (int rc = begin_ticket(hip_stream, &t, &st)) return rc;
    const int rc = issue_ticket(t, e, offset, &d_scalars, 1, n, window_begin, window_end, st);
    if (rc == BBGPU_ERR_ARG) set_error("bad window range [%d, %d)", window_begin, window_end);
    return rc ? rc : commit_ticket(t);
}

/* ---- bbgpu_plonk_verify_batch, bbgpu_plonk_verify_multi: verifier handles, and the GPU entries over one driver (the host twins and the argument checks
   are further up) ---- */
namespace {
struct VerifierHandle {
    host::VerifyKey K;
    VerifyRecord rec = {};                             // what the kernels read; base 0 (a call of several circuits sets it in its own copy)
    uint64_t shared_rows[host::VERIFY_MAX_SHARED * 8]; // the key's points and the generator as resident rows: Montgomery-261, canonical
};
std::vector<VerifierHandle*> g_verifiers; // under g_mu; never shrinks: a handle is an index
VerifierHandle* verifier_at(int v) { return v >= 0 && v < (int)g_verifiers.size() ? g_verifiers[v] : nullptr; } // null: no such handle
} // namespace

int bbgpu_plonk_verifier_create(size_t n, int widgets, const uint64_t vk[BBGPU_PLONK_VK_WORDS], const uint64_t g2_x[16])
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    VerifierHandle* H = new VerifierHandle();
    const char* why = "";
    if (int rc = host::verify_key_init(&H->K, n, widgets, vk, g2_x, &why)) {
        set_error("PLONK verifier: %s", why);
        delete H;
        return rc;
    }
    const host::VerifyKey& K = H->K;
    H->rec.log2n = (uint32_t)K.log2n;
    H->rec.widgets = (uint32_t)K.widgets;
    H->rec.num_vk = (uint32_t)K.num_vk;
    const Limbs9 root = host::limbs_m261(K.root), root_inv = host::limbs_m261(K.root_inv), n_inv = host::limbs_m261(K.n_inv);
    memcpy(H->rec.root, root.d, sizeof root.d);
    memcpy(H->rec.root_inv, root_inv.d, sizeof root_inv.d);
    memcpy(H->rec.n_inv, n_inv.d, sizeof n_inv.d);
    uint64_t pts[host::VERIFY_MAX_SHARED * 8];
    host::verify_shared_points(K, pts);
    for (int k = 0; k < K.num_shared(); k++) {
        if (k < K.num_vk && K.vk_inf[k]) H->rec.skip_mask |= 1u << k; // a stand-in row, scalar zero
        resident_row(pts + 8 * k, H->shared_rows + 8 * k);
    }
    for (size_t h = 0; h < g_verifiers.size(); h++)
        if (!g_verifiers[h]) {
            g_verifiers[h] = H;
            return (int)h;
        }
    g_verifiers.push_back(H);
    return (int)g_verifiers.size() - 1;
}

int bbgpu_plonk_verifier_destroy(int verifier)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (!verifier_at(verifier)) {
        set_error("unknown verifier handle %d", verifier);
        return BBGPU_ERR_ARG;
    }
    delete g_verifiers[verifier];
    g_verifiers[verifier] = nullptr;
    return BBGPU_OK;
}

// Both entries behind their argument checks: proof j is of H[circuit[j]], every handle under H[0]'s g2_x.  A call of one circuit (G == 1: circuit[] is
// not read) passes that circuit's record to the kernels as an argument; a call of several lays circuit[] and the records out on the device.
static int verify_run(const VerifierHandle* const* H, size_t G, const uint32_t* circuit, const uint64_t* proofs, size_t count, const uint64_t seed[4], int flags,
                      uint32_t* status, bbgpu_plonk_verify_report* out)
{
    if (int rc = ensure_init()) return rc;
    StageClock& clock = g_verify_clock;
    clock.begin();
    uint64_t sd[4];
    if (int rc = call_seed("PLONK verify", seed, sd)) return rc;
    host::verify_report_init(out, count, sd);
    const bool uniform = G == 1;
    // one staging buffer, every part a multiple of 64 bytes: the proofs | circuit[] | the records | rows of A: every circuit's shared rows, then nine
    // per proof | rows of B: two per proof | scalars of A, of B | the shared terms [slot][proof] | the statuses.  circuit[], the records (both empty when
    // the call is uniform) and the shared rows are neighbours there because they arrive in one copy.
    size_t T = 0, S_max = 0; // shared rows in all, the most of one circuit
    for (size_t c = 0; c < G; c++) {
        T += (size_t)H[c]->K.num_shared();
        S_max = std::max(S_max, (size_t)H[c]->K.num_shared());
    }
    const size_t na = T + host::VERIFY_OWN * count, nb = 2 * count;
    auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
    const size_t o_circuit = up64(count * BBGPU_PLONK_PROOF_WORDS * 8), o_records = o_circuit + (uniform ? 0 : up64(count * 4)),
                 o_rows_a = o_records + (uniform ? 0 : G * sizeof(VerifyRecord)), o_rows_b = o_rows_a + na * 64, o_scal_a = o_rows_b + nb * 64,
                 o_scal_b = o_scal_a + up64(na * 32), o_shared = o_scal_b + nb * 32, o_status = o_shared + up64(S_max * count * 32),
                 total = o_status + up64(count * 4);
    const size_t head_bytes = o_rows_a + T * 64 - o_circuit;
    static_assert(BBGPU_PLONK_VERIFY_MAX_BATCH * 4 + BBGPU_PLONK_VERIFY_MAX_CIRCUITS * (sizeof(VerifyRecord) + host::VERIFY_MAX_SHARED * 64) <= Context::HOST_CHUNK,
                  "circuit[], the records and the shared rows fit one pinned staging buffer");
    if (int rc = grow(&ctx().d_verify, &ctx().verify_cap, total)) return rc;
    uint8_t* base = reinterpret_cast<uint8_t*>(ctx().d_verify);
    uint32_t *d_rows_a = reinterpret_cast<uint32_t*>(base + o_rows_a), *d_rows_b = reinterpret_cast<uint32_t*>(base + o_rows_b);
    uint64_t *d_scal_a = reinterpret_cast<uint64_t*>(base + o_scal_a), *d_scal_b = reinterpret_cast<uint64_t*>(base + o_scal_b);
    uint64_t* d_shared = reinterpret_cast<uint64_t*>(base + o_shared);
    uint32_t* d_status = reinterpret_cast<uint32_t*>(base + o_status);
    VerifyCircuits C;
    if (uniform) {
        C.one = &H[0]->rec;
    } else {
        C.d_circuit = reinterpret_cast<const uint32_t*>(base + o_circuit);
        C.d_records = reinterpret_cast<const VerifyRecord*>(base + o_records);
        C.num_circuits = (int)G;
        C.max_shared = (int)S_max;
    }
    const hipStream_t st = ctx().stream;
    if (int rc = host_to_device(base, proofs, count * BBGPU_PLONK_PROOF_WORDS * 8, st)) return rc;
    // the head, built in one of the library's pinned staging buffers (host_to_device's ring), sent in one copy
    const int rc_head = stage_head(base + o_circuit, head_bytes, st, [&](uint8_t* h) {
        memset(h, 0, o_records - o_circuit);
        if (!uniform) memcpy(h, circuit, count * 4);
        VerifyRecord* rec = reinterpret_cast<VerifyRecord*>(h + (o_records - o_circuit));
        uint8_t* rows = h + (o_rows_a - o_circuit);
        size_t at = 0;
        for (size_t c = 0; c < G; c++) {
            if (!uniform) {
                rec[c] = H[c]->rec;
                rec[c].base = (uint32_t)at;
            }
            memcpy(rows + at * 64, H[c]->shared_rows, (size_t)H[c]->K.num_shared() * 64);
            at += (size_t)H[c]->K.num_shared();
        }
    });
    if (rc_head) return rc_head;
    VerifyDeviceBuffers B;
    B.proofs = reinterpret_cast<const uint64_t*>(base);
    B.rows_own = d_rows_a + T * 16;
    B.rows_other = d_rows_b;
    B.scal_own = d_scal_a + T * 4;
    B.scal_other = d_scal_b;
    B.shared = d_shared;
    B.status = d_status;
    if (int rc = plonk_verify_terms(C, sd, count, B, st)) return rc;
    HIPCHK(d2h_async(status, d_status, count * 4, st));
    HIPCHK(hipStreamSynchronize(st));
    clock.first_sync();
    host::verify_count_status(out, status);
    // A and B: two tickets in flight over the rows the kernel wrote, the scalars where the kernels left them
    const SrsEntry ea = transient_table(d_rows_a, na), eb = transient_table(d_rows_b, nb);
    const int rc_tail = host::verify_tail(out, H[0]->K.g2_x, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) -> int {
        const double t_fold = now_ms();
        if (int rc = plonk_verify_fold(C, d_shared, count, m, d_scal_a, st)) return rc;
        HIPCHK(hipStreamSynchronize(st)); // the tickets run on their slots' own streams
        const double t_msm = now_ms();
        clock.ms[2] += t_msm - t_fold;
        if (int rc = two_msms(ea, 0, d_scal_a, T + host::VERIFY_OWN * m, eb, 0, d_scal_b, 2 * m, a12, b12)) return rc;
        clock.ms[3] += now_ms() - t_msm;
        return BBGPU_OK;
    });
    clock.end();
    return rc_tail;
}

int bbgpu_plonk_verify_batch(int verifier, const uint64_t* proofs, size_t count, const uint64_t seed[4], int flags, uint32_t* status,
                             bbgpu_plonk_verify_report* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    if (int rc = verify_args(proofs, count, flags, status, out)) return rc;
    const VerifierHandle* H = verifier_at(verifier);
    if (!H) {
        set_error("unknown verifier handle %d", verifier);
        return BBGPU_ERR_ARG;
    }
    return verify_run(&H, 1, nullptr, proofs, count, seed, flags, status, out);
}

int bbgpu_plonk_verify_multi(const int* verifiers, int num_verifiers, const uint32_t* circuit, const uint64_t* proofs, size_t count, const uint64_t seed[4],
                             int flags, uint32_t* status, bbgpu_plonk_verify_report* out)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    if (int rc = verify_multi_args(verifiers, num_verifiers, "verifiers", circuit, proofs, count, flags, status, out)) return rc;
    const VerifierHandle* H[BBGPU_PLONK_VERIFY_MAX_CIRCUITS];
    for (int c = 0; c < num_verifiers; c++) {
        if (!(H[c] = verifier_at(verifiers[c]))) {
            set_error("unknown verifier handle %d (verifiers[%d])", verifiers[c], c);
            return BBGPU_ERR_ARG;
        }
        if (memcmp(H[c]->K.g2_x, H[0]->K.g2_x, sizeof H[0]->K.g2_x) != 0) {
            set_error("PLONK verify: verifiers[%d] (handle %d) and verifiers[0] (handle %d) hold different g2_x: one call, one reference string", c, verifiers[c],
                      verifiers[0]);
            return BBGPU_ERR_ARG;
        }
    }
    return verify_run(H, (size_t)num_verifiers, circuit, proofs, count, seed, flags, status, out);
}

int bbgpu_plonk_verify_last_timing(double ms_out[5])
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return g_verify_clock.read(ms_out);
}

/* ---- batched check of KZG openings (host_kzg_check_batch.hpp, kzg_check.hip) ---- */
static int kzg_check_refused(int rc, const char* why)
{
    set_error("KZG check: %s", why);
    return rc;
}
// the call of bbgpu_(host_)kzg_check_openings and its argument verdict
static int kzg_check_openings_call(host::KzgCheckCall* K, const uint64_t* commitments, const uint32_t* which, size_t num_commitments, const uint64_t* z,
                                   const uint64_t* y, const uint64_t* proofs, size_t count, const uint64_t* g2_x, int flags, const bbgpu_kzg_check_report* out)
{
    K->commitments = commitments;
    K->which = which;
    K->S = which ? num_commitments : 0;
    K->z = z;
    K->y = y;
    K->proofs = proofs;
    K->count = count;
    const char* why = "";
    if (int rc = host::kzg_check_args(*K, which == nullptr, num_commitments, g2_x, flags, out, &why)) return kzg_check_refused(rc, why);
    return BBGPU_OK;
}
// the same for bbgpu_(host_)kzg_check_open_all
static int kzg_check_open_all_call(host::KzgCheckCall* K, const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n,
                                   int batch, const uint64_t* g2_x, int flags, const bbgpu_kzg_check_report* out)
{
    if (!host::kzg_check_open_all_sizes_ok(n, stride, batch, &K->log2n))
        return kzg_check_refused(BBGPU_ERR_SIZE, "n a power of two, 1 <= batch <= 64, stride >= n and batch x n <= 2^20 are taken");
    K->commitments = commitments;
    K->S = (size_t)batch;
    K->y = values;
    K->y_stride = stride;
    K->proofs = proofs;
    K->count = (size_t)batch * n;
    K->open_all = true;
    const char* why = "";
    if (int rc = host::kzg_check_args(*K, false, (size_t)batch, g2_x, flags, out, &why)) return kzg_check_refused(rc, why);
    return BBGPU_OK;
}

int bbgpu_host_kzg_check_openings_batch(const uint64_t* commitments, const uint32_t* which, size_t num_commitments, const uint64_t* z, const uint64_t* y,
                                        const uint64_t* proofs, size_t count, const uint64_t g2_x[16], const uint64_t seed[4], int flags,
                                        bbgpu_kzg_check_report* report)
{
    host::KzgCheckCall K;
    if (int rc = kzg_check_openings_call(&K, commitments, which, num_commitments, z, y, proofs, count, g2_x, flags, report)) return rc;
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    return host::kzg_check_host(K, g2_x, sd, flags, report);
}
int bbgpu_host_kzg_check_open_all(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, int batch,
                                  const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    host::KzgCheckCall K;
    if (int rc = kzg_check_open_all_call(&K, commitments, values, stride, proofs, n, batch, g2_x, flags, report)) return rc;
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    return host::kzg_check_host(K, g2_x, sd, flags, report);
}

// a point in the reference's format as a resident row (Montgomery-261, canonical); the generator for the point at infinity.  Returns the infinity flag.
static bool kzg_check_resident_row(const uint64_t* p, uint64_t out[8])
{
    uint64_t pt[8];
    const bool inf = host::kzg_row(p, pt);
    resident_row(pt, out);
    return inf;
}

// The three forms behind their argument checks, modelled on verify_run: upload, k_kzg_claims, ONE synchronisation before the findings are read, then per
// round the fold and two tickets over the rows as transient tables, and the shared host tail.
static int kzg_check_run(const host::KzgCheckCall& K, const uint64_t g2_x[16], const uint64_t* seed, int flags, bbgpu_kzg_check_report* out)
{
    if (int rc = ensure_init()) return rc;
    StageClock& clock = g_kzg_check_clock;
    clock.begin();
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    host::kzg_report_init(out, K.count, sd);
    const size_t count = K.count, S = K.S, H = K.head(), per = K.per(), na = H + per * count, nb = per * count;
    const bool per_claim = !K.shared();
    // one staging buffer, every part at a multiple of 32 bytes (the kernels read and write 16 bytes at a time): the proofs | y | z | the per-claim commitments | the labels | the findings | the rows: the
    // shared commitments, G, then the claims' | the scalars of A, of B | the terms rho y, rho | the partial sums of the fold.  The findings and the head
    // of the rows are neighbours because they arrive in one copy.
    auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
    const size_t o_y = count * 64, o_z = o_y + count * 32, o_commit = o_z + (K.open_all ? 0 : count * 32), o_which = o_commit + (per_claim ? count * 64 : 0),
                 o_find = o_which + (K.which ? up64(count * 4) : 0), o_rows = o_find + 64, o_scal_a = o_rows + na * 64, o_scal_b = o_scal_a + up64(na * 32),
                 o_term_y = o_scal_b + up64(nb * 32), o_term_rho = o_term_y + count * 32, o_partial = o_term_rho + (per_claim ? 0 : count * 32),
                 total = o_partial + H * KZG_FOLD_MAX_RANGES * 32;
    static_assert(64 + (BBGPU_KZG_CHECK_MAX_COMMITMENTS + 1) * 64 <= Context::HOST_CHUNK, "the findings and the shared rows fit one pinned staging buffer");
    if (int rc = grow(&ctx().d_kzg_check, &ctx().kzg_check_cap, total)) return rc;
    uint8_t* base = reinterpret_cast<uint8_t*>(ctx().d_kzg_check);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(base + o_rows);
    uint64_t *d_scal_a = reinterpret_cast<uint64_t*>(base + o_scal_a), *d_scal_b = reinterpret_cast<uint64_t*>(base + o_scal_b);
    KzgCheckBuffers B{};
    B.proofs = reinterpret_cast<const uint64_t*>(base);
    B.y = reinterpret_cast<const uint64_t*>(base + o_y);
    B.z = K.open_all ? nullptr : reinterpret_cast<const uint64_t*>(base + o_z);
    B.commitments = per_claim ? reinterpret_cast<const uint64_t*>(base + o_commit) : nullptr;
    B.which = K.which ? reinterpret_cast<const uint32_t*>(base + o_which) : nullptr;
    B.rows = d_rows + H * 16;
    B.scal_a = d_scal_a + H * 4;
    B.scal_b = d_scal_b;
    B.term_y = reinterpret_cast<uint64_t*>(base + o_term_y);
    B.term_rho = per_claim ? nullptr : reinterpret_cast<uint64_t*>(base + o_term_rho);
    B.partial = reinterpret_cast<uint64_t*>(base + o_partial);
    B.find = reinterpret_cast<KzgFindings*>(base + o_find);
    const hipStream_t st = ctx().stream;
    if (int rc = host_to_device(base, K.proofs, count * 64, st)) return rc;
    if (K.open_all && K.y_stride != ((size_t)1 << K.log2n)) { // the values of each polynomial, without the caller's padding
        const size_t n = (size_t)1 << K.log2n;
        for (size_t b = 0; b < S; b++)
            if (int rc = host_to_device(base + o_y + b * n * 32, K.y + b * K.y_stride * 4, n * 32, st)) return rc;
    } else if (int rc = host_to_device(base + o_y, K.y, count * 32, st)) {
        return rc;
    }
    if (!K.open_all)
        if (int rc = host_to_device(base + o_z, K.z, count * 32, st)) return rc;
    if (per_claim)
        if (int rc = host_to_device(base + o_commit, K.commitments, count * 64, st)) return rc;
    if (K.which)
        if (int rc = host_to_device(base + o_which, K.which, count * 4, st)) return rc;
    uint64_t shared_bad, shared_first, skip_mask = 0;
    host::kzg_shared_findings(K, &shared_bad, &shared_first);
    // the head, built in one of the library's pinned staging buffers (host_to_device's ring), sent in one copy: the findings' start, the shared rows, G
    const int rc_head = stage_head(base + o_find, 64 + H * 64, st, [&](uint8_t* h) {
        memset(h, 0, 64);
        const KzgFindings init = { 0, ~0ull };
        memcpy(h, &init, sizeof init);
        uint64_t* rows = reinterpret_cast<uint64_t*>(h + 64);
        for (size_t c = 0; c < S; c++)
            if (kzg_check_resident_row(K.commitments + 8 * c, rows + 8 * c)) skip_mask |= 1ull << c;
        const uint64_t inf[8] = { 0, 0, 0, 0, 0, 0, 0, 1ull << 63 };
        (void)kzg_check_resident_row(inf, rows + 8 * S); // the generator
    });
    if (rc_head) return rc_head;
    Limbs9 omega{}, step{};
    if (K.open_all) {
        const host::Fr w = host::fr_root_of_unity(K.log2n);
        omega = host::limbs_m261(w);
        step = host::limbs_m261(host::fr_pow(w, (uint64_t)kzg_check_claim_threads(count) & (((uint64_t)1 << K.log2n) - 1)));
    }
    if (int rc = kzg_check_claims(B, sd, count, per_claim, K.open_all, K.log2n, omega.d, step.d, st)) return rc;
    KzgFindings got = { 0, ~0ull };
    HIPCHK(d2h_async(&got, B.find, sizeof got, st));
    HIPCHK(hipStreamSynchronize(st));
    clock.first_sync();
    host::kzg_report_findings(out, shared_bad, shared_first, got.bad_points, got.first_key);
    int rc_tail = BBGPU_OK;
    if (!out->bad_points) {
        // A and B: two tickets in flight over ONE transient table (the rows written above; no window tables), A from its head, B from the first claim on
        const SrsEntry ea = transient_table(d_rows, na), eb = transient_table(d_rows + H * 16, nb);
        rc_tail = host::kzg_check_tail(out, g2_x, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) -> int {
            const double t_fold = now_ms();
            if (int rc = kzg_check_fold(B, m, S, K.log2n, skip_mask, d_scal_a, st)) return rc;
            HIPCHK(hipStreamSynchronize(st)); // the tickets run on their slots' own streams
            const double t_msm = now_ms();
            clock.ms[2] += t_msm - t_fold;
            if (int rc = two_msms(ea, 0, d_scal_a, H + per * m, eb, 0, d_scal_b, per * m, a12, b12)) return rc;
            clock.ms[3] += now_ms() - t_msm;
            return BBGPU_OK;
        });
    }
    clock.end();
    return rc_tail;
}

int bbgpu_kzg_check_openings(const uint64_t* commitments, const uint32_t* which, size_t num_commitments, const uint64_t* z, const uint64_t* y,
                             const uint64_t* proofs, size_t count, const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgCheckCall K;
    if (int rc = kzg_check_openings_call(&K, commitments, which, num_commitments, z, y, proofs, count, g2_x, flags, report)) return rc;
    return kzg_check_run(K, g2_x, seed, flags, report);
}
int bbgpu_kzg_check_open_all(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, int batch,
                             const uint64_t g2_x[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgCheckCall K;
    if (int rc = kzg_check_open_all_call(&K, commitments, values, stride, proofs, n, batch, g2_x, flags, report)) return rc;
    return kzg_check_run(K, g2_x, seed, flags, report);
}
/* ---- check of KZG cell proofs (host_kzg_check_cells.hpp, kzg_check_cells.hip) ---- */
// the call of bbgpu_(host_)kzg_check_cells and its argument verdict
static int kzg_cells_labelled_call(host::KzgCellsCall* K, const uint64_t* commitments, size_t num_commitments, const uint32_t* which, const uint32_t* cell,
                                   const uint64_t* values, const uint64_t* proofs, size_t count, size_t n, size_t coset, const uint64_t* g1_head,
                                   const uint64_t* g2_xl, int flags, const bbgpu_kzg_check_report* out,
                                   size_t max_commitments = BBGPU_KZG_CHECK_MAX_COMMITMENTS)
{
    K->commitments = commitments;
    K->S = num_commitments;
    K->which = which;
    K->cell = cell;
    K->values = values;
    K->proofs = proofs;
    K->head = g1_head;
    K->count = count;
    char why[160];
    if (int rc = host::kzg_cells_args(K, n, coset, 0, g2_xl, flags, out, why, sizeof why, max_commitments)) return kzg_check_refused(rc, why);
    return BBGPU_OK;
}
// the same for bbgpu_(host_)kzg_check_open_cosets
static int kzg_cells_open_cosets_call(host::KzgCellsCall* K, const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n,
                                      size_t coset, int batch, const uint64_t* g1_head, const uint64_t* g2_xl, int flags, const bbgpu_kzg_check_report* out,
                                      size_t max_commitments = BBGPU_KZG_CHECK_MAX_COMMITMENTS)
{
    K->commitments = commitments;
    K->values = values;
    K->proofs = proofs;
    K->head = g1_head;
    K->cosets = true;
    K->stride = stride;
    char why[160];
    if (int rc = host::kzg_cells_args(K, n, coset, batch, g2_xl, flags, out, why, sizeof why, max_commitments)) return kzg_check_refused(rc, why);
    return BBGPU_OK;
}

int bbgpu_host_kzg_check_cells(const uint64_t* commitments, size_t num_commitments, const uint32_t* which, const uint32_t* cell, const uint64_t* values,
                               const uint64_t* proofs, size_t count, size_t n, size_t coset, const uint64_t* g1_head, const uint64_t g2_xl[16],
                               const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    host::KzgCellsCall K;
    if (int rc = kzg_cells_labelled_call(&K, commitments, num_commitments, which, cell, values, proofs, count, n, coset, g1_head, g2_xl, flags, report)) return rc;
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    return host::kzg_cells_host(K, g2_xl, sd, flags, report);
}
int bbgpu_host_kzg_check_open_cosets(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, size_t coset,
                                     int batch, const uint64_t* g1_head, const uint64_t g2_xl[16], const uint64_t seed[4], int flags,
                                     bbgpu_kzg_check_report* report)
{
    host::KzgCellsCall K;
    if (int rc = kzg_cells_open_cosets_call(&K, commitments, values, stride, proofs, n, coset, batch, g1_head, g2_xl, flags, report)) return rc;
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    return host::kzg_cells_host(K, g2_xl, sd, flags, report);
}
// the layout twins: the same plain loops behind the cap of BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS
int bbgpu_host_kzg_check_cells_layout(const uint64_t* commitments, size_t num_commitments, const uint32_t* which, const uint32_t* cell, const uint64_t* values,
                                      const uint64_t* proofs, size_t count, size_t n, size_t coset, const uint64_t* g1_head, const uint64_t g2_xl[16],
                                      const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    host::KzgCellsCall K;
    if (int rc = kzg_cells_labelled_call(&K, commitments, num_commitments, which, cell, values, proofs, count, n, coset, g1_head, g2_xl, flags, report,
                                         BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS))
        return rc;
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    return host::kzg_cells_host(K, g2_xl, sd, flags, report);
}
int bbgpu_host_kzg_check_open_cosets_layout(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, size_t coset,
                                            int batch, const uint64_t* g1_head, const uint64_t g2_xl[16], const uint64_t seed[4], int flags,
                                            bbgpu_kzg_check_report* report)
{
    host::KzgCellsCall K;
    if (int rc = kzg_cells_open_cosets_call(&K, commitments, values, stride, proofs, n, coset, batch, g1_head, g2_xl, flags, report,
                                            BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS))
        return rc;
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    return host::kzg_cells_host(K, g2_xl, sd, flags, report);
}
int bbgpu_host_kzg_cells_key_check(const uint64_t* g1_head, size_t coset, const uint64_t g2_x[16], const uint64_t g2_xl[16], int* ok)
{
    if (coset < 1 || coset > BBGPU_KZG_OPEN_COSETS_MAX_COSET || (coset & (coset - 1)))
        return kzg_check_refused(BBGPU_ERR_SIZE, "the cells' key: coset a power of two in 1 .. 64 is taken");
    if (!g1_head || !g2_x || !g2_xl || !ok) return kzg_check_refused(BBGPU_ERR_ARG, "the cells' key: null g1_head / g2_x / g2_xl / ok");
    *ok = host::kzg_cells_key_ok(g1_head, coset, g2_x, g2_xl) ? 1 : 0;
    return BBGPU_OK;
}

// Both forms behind their argument checks, modelled on kzg_check_run: upload, k_kzg_cells and k_kzg_cell_coefficients, ONE synchronisation before the
// findings are read, then per round the fold and two tickets over the rows as transient tables, and the shared host tail with [x^l] G2.
// layout: the entries of up to 2^16 commitments.  Their commitments go up as they are and k_kzg_layout_commitments makes the rows, the skip bits and the
// findings; the table starts with P_0 .. P_(l-1), which still arrive with the head, and the commitments follow -- a sum does not depend on the order of
// its rows --; k_kzg_cells_fold keeps the l slots of P_i and the grouped fold writes the S scalars behind them.
static int kzg_cells_run(const host::KzgCellsCall& K, const uint64_t g2_xl[16], const uint64_t* seed, int flags, bbgpu_kzg_check_report* out, bool layout = false)
{
    if (int rc = ensure_init()) return rc;
    StageClock& clock = g_kzg_check_clock;
    clock.begin();
    uint64_t sd[4];
    if (int rc = call_seed("KZG check", seed, sd)) return rc;
    host::kzg_report_init(out, K.count, sd);
    const size_t count = K.count, S = K.S, l = K.l(), n = (size_t)1 << K.log2n, H = K.rows_head(), na = H + count;
    const size_t nvals = K.cosets ? S * n : count * l;
    const size_t HC = layout ? l : H, row_c = layout ? l : 0, row_p = layout ? 0 : S; // the rows the head brings; the first commitment's and P_0's row
    // one staging buffer, every part at a multiple of 64 bytes: the proofs | the values | the labels | the cell indices | the roots | the findings | the
    // rows: the shared commitments, P_0 .. P_(l-1), then the cells' | the scalars of A, of B | rho | the terms | the partial sums of the fold.  The roots,
    // the findings and the head of the rows are neighbours because they arrive in one copy.  The layout entries add: the commitments' raw words | the skip
    // bits | and in the labelled form the S counters | the S + 1 starts of the lists | the S + 1 first pieces | the permutation | then the sums of the
    // pieces: 76 bytes per commitment and 4 + 1/32 per cell (labelled), 64 + 1/8 + 32 ceil(m / 1024) per commitment (open-cosets).
    auto up64 = [](size_t b) { return (b + 63) & ~(size_t)63; };
    constexpr size_t ROOTS = (KZG_CELLS_MAX_COSET * sizeof(Limbs9) + 63) / 64 * 64;
    const size_t o_values = count * 64, o_which = o_values + nvals * 32, o_cell = o_which + (K.cosets ? 0 : up64(count * 4)),
                 o_roots = o_cell + (K.cosets ? 0 : up64(count * 4)), o_find = o_roots + ROOTS, o_rows = o_find + 64, o_scal_a = o_rows + na * 64,
                 o_scal_b = o_scal_a + up64(na * 32), o_rho = o_scal_b + up64(count * 32), o_term = o_rho + count * 32, o_partial = o_term + count * l * 32,
                 o_commit = o_partial + HC * KZG_FOLD_MAX_RANGES * 32, o_skip = o_commit + (layout ? S * 64 : 0),
                 o_cnt = o_skip + (layout ? up64((S + 63) / 64 * 8) : 0), o_off = o_cnt + (layout && !K.cosets ? up64(S * 4) : 0),
                 o_poff = o_off + (layout && !K.cosets ? up64((S + 1) * 4) : 0), o_perm = o_poff + (layout && !K.cosets ? up64((S + 1) * 4) : 0),
                 o_pieces = o_perm + (layout && !K.cosets ? up64(count * 4) : 0),
                 total = o_pieces + (layout ? kzg_layout_max_pieces(count, S, K.log2n - K.log2l, K.cosets) * 32 : 0);
    static_assert(ROOTS + 64 + (BBGPU_KZG_CHECK_MAX_COMMITMENTS + KZG_CELLS_MAX_COSET) * 64 <= Context::HOST_CHUNK, "the head fits one pinned staging buffer");
    static_assert(KZG_CELLS_MAX_COSET == BBGPU_KZG_OPEN_COSETS_MAX_COSET, "one bound on the coset size");
    if (int rc = grow(&ctx().d_kzg_check, &ctx().kzg_check_cap, total)) return rc;
    uint8_t* base = reinterpret_cast<uint8_t*>(ctx().d_kzg_check);
    uint32_t* d_rows = reinterpret_cast<uint32_t*>(base + o_rows);
    uint64_t *d_scal_a = reinterpret_cast<uint64_t*>(base + o_scal_a), *d_scal_b = reinterpret_cast<uint64_t*>(base + o_scal_b);
    KzgCellsBuffers B{};
    B.proofs = reinterpret_cast<const uint64_t*>(base);
    B.values = reinterpret_cast<const uint64_t*>(base + o_values);
    B.which = K.cosets ? nullptr : reinterpret_cast<const uint32_t*>(base + o_which);
    B.cell = K.cosets ? nullptr : reinterpret_cast<const uint32_t*>(base + o_cell);
    B.rows = d_rows + H * 16;
    B.scal_a = d_scal_a + H * 4;
    B.scal_b = d_scal_b;
    B.term_rho = reinterpret_cast<uint64_t*>(base + o_rho);
    B.term = reinterpret_cast<uint64_t*>(base + o_term);
    B.partial = reinterpret_cast<uint64_t*>(base + o_partial);
    B.roots = reinterpret_cast<const uint32_t*>(base + o_roots);
    B.find = reinterpret_cast<KzgFindings*>(base + o_find);
    KzgLayoutBuffers L{};
    L.commitments = reinterpret_cast<const uint64_t*>(base + o_commit);
    L.which = B.which;
    L.rows = d_rows + row_c * 16;
    L.skip = reinterpret_cast<uint64_t*>(base + o_skip);
    L.find = B.find + 1; // the second 16 bytes of the findings' 64
    L.cnt = reinterpret_cast<uint32_t*>(base + o_cnt);
    L.off = reinterpret_cast<uint32_t*>(base + o_off);
    L.poff = reinterpret_cast<uint32_t*>(base + o_poff);
    L.perm = reinterpret_cast<uint32_t*>(base + o_perm);
    L.partial = reinterpret_cast<uint64_t*>(base + o_pieces);
    const hipStream_t st = ctx().stream;
    if (int rc = host_to_device(base, K.proofs, count * 64, st)) return rc;
    if (K.cosets && K.stride != n) { // the transform of each polynomial, without the caller's padding
        for (size_t b = 0; b < S; b++)
            if (int rc = host_to_device(base + o_values + b * n * 32, K.values + b * K.stride * 4, n * 32, st)) return rc;
    } else if (int rc = host_to_device(base + o_values, K.values, nvals * 32, st)) {
        return rc;
    }
    if (!K.cosets) {
        if (int rc = host_to_device(base + o_which, K.which, count * 4, st)) return rc;
        if (int rc = host_to_device(base + o_cell, K.cell, count * 4, st)) return rc;
    }
    uint64_t shared_bad = 0, shared_first = UINT64_MAX, skip_mask = 0;
    if (layout) {
        if (int rc = host_to_device(base + o_commit, K.commitments, S * 64, st)) return rc;
    } else {
        for (size_t c = 0; c < S; c++)
            if (!host::g1_words_acceptable(K.commitments + 8 * c) && shared_bad++ == 0) shared_first = c;
    }
    const host::KzgCellsDomain D = host::kzg_cells_domain(K.log2n, K.log2l);
    // the head, built in one of the library's pinned staging buffers (host_to_device's ring), sent in one copy: the roots zeta^-e, the findings' start, the
    // shared rows, P_0 .. P_(l-1)
    const int rc_head = stage_head(base + o_roots, ROOTS + 64 + HC * 64, st, [&](uint8_t* h) {
        memset(h, 0, ROOTS + 64);
        for (size_t e = 0; e < l; e++) {
            const Limbs9 z = host::limbs_m261(D.zeta_inv[e]);
            memcpy(h + e * sizeof(Limbs9), z.d, sizeof(Limbs9));
        }
        const KzgFindings init[2] = { { 0, ~0ull }, { 0, ~0ull } }; // the cells', the layout entries' commitments'
        memcpy(h + ROOTS, init, sizeof init);
        uint64_t* rows = reinterpret_cast<uint64_t*>(h + ROOTS + 64);
        for (size_t c = 0; c < S && !layout; c++)
            if (kzg_check_resident_row(K.commitments + 8 * c, rows + 8 * c)) skip_mask |= 1ull << c;
        for (size_t i = 0; i < l; i++) (void)kzg_check_resident_row(K.head + 8 * i, rows + 8 * (row_p + i)); // finite: the arguments were checked
    });
    if (rc_head) return rc_head;
    float group_ms = 0, fold_ms = 0;
    bool fold_timed = false;
    if (layout)
        if (int rc = kzg_layout_group(L, count, S, st, ctx().timing ? &group_ms : nullptr)) return rc;
    if (int rc = kzg_cells_claims(B, sd, count, K.log2n, K.log2l, host::limbs_m261(D.psi).d, st)) return rc;
    float coef_ms = 0;
    if (int rc = kzg_cells_coefficients(B, count, K.log2n, K.log2l, host::limbs_m261(D.omega_inv).d,
                                        host::limbs_m261(host::fr_mul(D.l_inv, host::fr_from_u64(32))).d, st, ctx().timing ? &coef_ms : nullptr))
        return rc;
    KzgFindings got[2] = { { 0, ~0ull }, { 0, ~0ull } };
    HIPCHK(d2h_async(got, B.find, layout ? sizeof got : sizeof got[0], st));
    HIPCHK(hipStreamSynchronize(st));
    clock.first_sync();
    if (layout) {
        shared_bad = got[1].bad_points;
        shared_first = got[1].first_key;
    }
    host::kzg_report_findings(out, shared_bad, shared_first, got[0].bad_points, got[0].first_key);
    int rc_tail = BBGPU_OK;
    if (!out->bad_points) {
        // A and B: two tickets in flight over ONE transient table, A from its head, B from the first cell on
        const SrsEntry ea = transient_table(d_rows, na), eb = transient_table(d_rows + H * 16, count);
        rc_tail = host::kzg_check_tail(out, g2_xl, flags, [&](size_t m, uint64_t* a12, uint64_t* b12) -> int {
            const double t_fold = now_ms();
            if (int rc = kzg_cells_fold(B, m, layout ? 0 : S, K.log2n, K.log2l, skip_mask, d_scal_a, st)) return rc;
            if (layout) {
                float* ms = ctx().timing && !fold_timed ? &fold_ms : nullptr; // the first round's
                fold_timed = true;
                if (int rc = kzg_layout_fold(L, B.term_rho, m, count, S, K.log2n - K.log2l, d_scal_a + row_c * 4, st, ms)) return rc;
            }
            HIPCHK(hipStreamSynchronize(st)); // the tickets run on their slots' own streams
            const double t_msm = now_ms();
            clock.ms[2] += t_msm - t_fold;
            if (int rc = two_msms(ea, 0, d_scal_a, H + m, eb, 0, d_scal_b, m, a12, b12)) return rc;
            clock.ms[3] += now_ms() - t_msm;
            return BBGPU_OK;
        });
    }
    clock.end();
    if (ctx().timing) { // bbgpu_last_timing: index 0 the coefficient kernel alone (set last: the tickets' waits write their own)
        ctx().last.count = layout ? 3 : 1;
        ctx().last.ms[0] = coef_ms;
        if (layout) { // 1: k_kzg_layout_commitments and the grouping; 2: the grouped fold of the first round
            ctx().last.ms[1] = group_ms;
            ctx().last.ms[2] = fold_ms;
        }
    }
    return rc_tail;
}

int bbgpu_kzg_check_cells(const uint64_t* commitments, size_t num_commitments, const uint32_t* which, const uint32_t* cell, const uint64_t* values,
                          const uint64_t* proofs, size_t count, size_t n, size_t coset, const uint64_t* g1_head, const uint64_t g2_xl[16],
                          const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgCellsCall K;
    if (int rc = kzg_cells_labelled_call(&K, commitments, num_commitments, which, cell, values, proofs, count, n, coset, g1_head, g2_xl, flags, report)) return rc;
    return kzg_cells_run(K, g2_xl, seed, flags, report);
}
int bbgpu_kzg_check_open_cosets(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, size_t coset, int batch,
                                const uint64_t* g1_head, const uint64_t g2_xl[16], const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgCellsCall K;
    if (int rc = kzg_cells_open_cosets_call(&K, commitments, values, stride, proofs, n, coset, batch, g1_head, g2_xl, flags, report)) return rc;
    return kzg_cells_run(K, g2_xl, seed, flags, report);
}
int bbgpu_kzg_check_cells_layout(const uint64_t* commitments, size_t num_commitments, const uint32_t* which, const uint32_t* cell, const uint64_t* values,
                                 const uint64_t* proofs, size_t count, size_t n, size_t coset, const uint64_t* g1_head, const uint64_t g2_xl[16],
                                 const uint64_t seed[4], int flags, bbgpu_kzg_check_report* report)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgCellsCall K;
    if (int rc = kzg_cells_labelled_call(&K, commitments, num_commitments, which, cell, values, proofs, count, n, coset, g1_head, g2_xl, flags, report,
                                         BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS))
        return rc;
    return kzg_cells_run(K, g2_xl, seed, flags, report, true);
}
int bbgpu_kzg_check_open_cosets_layout(const uint64_t* commitments, const uint64_t* values, size_t stride, const uint64_t* proofs, size_t n, size_t coset,
                                       int batch, const uint64_t* g1_head, const uint64_t g2_xl[16], const uint64_t seed[4], int flags,
                                       bbgpu_kzg_check_report* report)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgCellsCall K;
    if (int rc = kzg_cells_open_cosets_call(&K, commitments, values, stride, proofs, n, coset, batch, g1_head, g2_xl, flags, report,
                                            BBGPU_KZG_CHECK_MAX_LAYOUT_COMMITMENTS))
        return rc;
    return kzg_cells_run(K, g2_xl, seed, flags, report, true);
}
int bbgpu_kzg_check_last_timing(double ms_out[5])
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    return g_kzg_check_clock.read(ms_out);
}

/* ---- polynomials recovered from a subset of their cells (host_kzg_recover_cells.hpp, kzg_recover_cells.hip) ---- */
int bbgpu_host_kzg_recover_cells(const uint32_t* cell, size_t count, const uint64_t* values, size_t n, size_t coset, size_t degree_bound, int batch,
                                 uint64_t* coeffs_out, size_t stride_elems, uint64_t* values_out, bbgpu_kzg_recover_report* report)
{
    host::KzgRecoverShape S;
    char why[320];
    int rc = host::kzg_recover_verdict("host kzg_recover_cells", cell, count, values, n, coset, degree_bound, batch, coeffs_out, stride_elems, report, &S, why,
                                       sizeof why);
    if (rc == BBGPU_OK) rc = host::kzg_recover_cells_host(S, cell, count, values, degree_bound, batch, coeffs_out, stride_elems, values_out, report, why, sizeof why);
    if (rc) set_error("%s", why);
    return rc;
}

// The findings of the three recoveries on the host: ~0 goes up before the kernels, their minima come down after them, split for the report functions.
struct RecoverFound {
    std::vector<RecoverFindings> both;
    std::vector<uint64_t> first_bad, first_bug;
    explicit RecoverFound(int batch) : both((size_t)batch, RecoverFindings{ ~0ull, ~0ull }), first_bad((size_t)batch), first_bug((size_t)batch) {}
    int begin(void* d_find, hipStream_t st) { return host_to_device(d_find, both.data(), both.size() * sizeof(RecoverFindings), st); }
    int end(const void* d_find, hipStream_t st)
    {
        if (int rc = device_to_host_sync(both.data(), d_find, both.size() * sizeof(RecoverFindings), st)) return rc;
        for (size_t b = 0; b < both.size(); b++) {
            first_bad[b] = both[b].first_bad;
            first_bug[b] = both[b].first_bug;
        }
        return BBGPU_OK;
    }
};

// What bbgpu_kzg_recover_cells and bbgpu_kzg_recover_cells_each do once z (d_z) and z' x 2^-5 (d_zc) stand, z_elems elements each, and event 1 can be
// marked: the batch inversion, scatter and IFFT, coset FFT, divide, coset IFFT and tail, the forward transform of the copy if there is one, and the
// findings on the host.  Events 1 .. 5 are marked here; recover_cells_timing reads them once the caller has nothing left that can fail.
static int recover_back_end(const RecoverLists& L, const uint64_t* d_vals, uint64_t* d_z, uint64_t* d_zc, size_t z_elems, size_t n, int log2n, int log2l,
                            size_t degree_bound, int batch, uint64_t* d_coeffs_out, size_t stride_elems, uint64_t* d_copy, RecoverFindings* d_find,
                            RecoverFound& F, StageEvents<6>& ev, void* hip_stream)
{
    const hipStream_t st = (hipStream_t)hip_stream;
    if (int rc = ev.mark(1, st)) return rc;
    if (int rc = bbgpu_fr_batch_invert_device(d_zc, z_elems, hip_stream)) return rc; // z' is never zero: g^n != 1
    if (int rc = ev.mark(2, st)) return rc;
    if (int rc = kzg_recover_scatter(d_vals, L, d_z, log2n, log2l, batch, d_coeffs_out, stride_elems, st)) return rc;
    if (int rc = bbgpu_ntt_device_batch(d_coeffs_out, n, stride_elems, batch, BBGPU_IFFT, nullptr, hip_stream)) return rc;
    if (int rc = ev.mark(3, st)) return rc;
    if (int rc = bbgpu_ntt_device_batch(d_coeffs_out, n, stride_elems, batch, BBGPU_COSET_FFT, nullptr, hip_stream)) return rc;
    if (int rc = kzg_recover_divide(d_coeffs_out, stride_elems, batch, d_zc, L, log2n, log2l, st)) return rc;
    if (int rc = bbgpu_ntt_device_batch(d_coeffs_out, n, stride_elems, batch, BBGPU_COSET_IFFT, nullptr, hip_stream)) return rc;
    if (int rc = kzg_recover_tail(d_coeffs_out, stride_elems, batch, d_copy, log2n, log2l, degree_bound, L, d_find, st)) return rc;
    if (int rc = ev.mark(4, st)) return rc;
    if (d_copy) {
        if (int rc = bbgpu_ntt_device_batch(d_copy, n, n, batch, BBGPU_FFT, nullptr, hip_stream)) return rc;
        if (int rc = ev.mark(5, st)) return rc;
    }
    return F.end(d_find, st);
}
// bbgpu_last_timing of both: index 0 what made z and z' (the caller's, between events 0 and 1), 1 scatter and IFFT, 2 coset FFT, divide, coset IFFT and
// tail, 3 the forward transform (if asked for)
static int recover_cells_timing(StageEvents<6>& ev, bool forward)
{
    if (!ev.on) return BBGPU_OK;
    ctx().last.count = forward ? 4 : 3;
    if (int rc = ev.ms(0, 1, &ctx().last.ms[0])) return rc;
    if (int rc = ev.ms(2, 3, &ctx().last.ms[1])) return rc;
    if (int rc = ev.ms(3, 4, &ctx().last.ms[2])) return rc;
    return forward ? ev.ms(4, 5, &ctx().last.ms[3]) : BBGPU_OK;
}

int bbgpu_kzg_recover_cells(const uint32_t* cell, size_t count, const uint64_t* values, size_t n, size_t coset, size_t degree_bound, int batch,
                            uint64_t* d_coeffs_out, size_t stride_elems, uint64_t* values_out, bbgpu_kzg_recover_report* report, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgRecoverShape S;
    char why[320];
    if (int rc = host::kzg_recover_verdict("kzg_recover_cells", cell, count, values, n, coset, degree_bound, batch, d_coeffs_out, stride_elems, report, &S, why,
                                           sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    const size_t m = S.m, mu = S.mu, present = count * coset, B = (size_t)batch;
    StageEvents<6> ev; // the stage boundaries of bbgpu_last_timing
    if (int rc = ev.create(ctx().timing != 0)) return rc;
    // the offsets b count, batch times mu, the cell list and the missing cells (ascending) in one array | z, z' and the roots of the missing cells | the
    // values | the findings | the copy the forward transform works in
    DevBuf lists, z, vals, find, copy;
    const size_t list_words = (B + 1) + B + m;
    HIPCHK(dev_malloc(&lists.p, list_words * 4));
    HIPCHK(dev_malloc(&z.p, 2 * m * 32 + mu * sizeof(Limbs9)));
    HIPCHK(dev_malloc(&vals.p, B * present * 32));
    HIPCHK(dev_malloc(&find.p, B * sizeof(RecoverFindings)));
    if (values_out) HIPCHK(dev_malloc(&copy.p, B * n * 32));
    std::vector<uint32_t> all(list_words);
    for (size_t b = 0; b <= B; b++) all[b] = (uint32_t)(b * count);
    std::fill_n(all.begin() + (B + 1), B, (uint32_t)mu);
    std::copy(cell, cell + count, all.begin() + (2 * B + 1));
    std::copy(S.missing.begin(), S.missing.end(), all.begin() + (2 * B + 1 + count));
    RecoverLists L{}; // mask and strides zero: one list of cells, one row of missing cells, one z and one z' for every polynomial
    L.d_off = lists.as<uint32_t>();
    L.d_mu = L.d_off + B + 1;
    L.d_cell = L.d_mu + B;
    L.d_missing = L.d_cell + count;
    uint64_t *d_z = z.as<uint64_t>(), *d_zc = d_z + 4 * m;
    uint32_t* d_roots = reinterpret_cast<uint32_t*>(d_zc + 4 * m);
    RecoverFound F(batch);
    if (int rc = host_to_device(lists.p, all.data(), list_words * 4, st)) return rc;
    if (int rc = F.begin(find.p, st)) return rc;
    if (int rc = host_to_device(vals.p, values, B * present * 32, st)) return rc;
    if (int rc = ev.mark(0, st)) return rc;
    if (int rc = kzg_recover_vanish(L.d_missing, mu, S.log2n, S.log2l, d_roots, d_z, d_zc, st)) return rc;
    if (int rc = recover_back_end(L, vals.as<uint64_t>(), d_z, d_zc, m, n, S.log2n, S.log2l, degree_bound, batch, d_coeffs_out, stride_elems, copy.as<uint64_t>(),
                                  find.as<RecoverFindings>(), F, ev, hip_stream))
        return rc;
    if (int rc = host::kzg_recover_report("kzg_recover_cells", F.first_bad.data(), F.first_bug.data(), batch, mu, report, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (values_out)
        if (int rc = device_to_host_sync(values_out, copy.p, B * n * 32, st)) return rc;
    return recover_cells_timing(ev, values_out != nullptr);
}

/* ---- the same for polynomials whose cell sets differ, at any n / l (host_kzg_recover_each.hpp, kzg_recover_each.hip) ---- */
int bbgpu_host_kzg_recover_cells_each(const uint32_t* cell_offsets, const uint32_t* cell, const uint64_t* values, size_t n, size_t coset, size_t degree_bound,
                                      int batch, uint64_t* coeffs_out, size_t stride_elems, uint64_t* values_out, uint64_t* first_bad_out,
                                      bbgpu_kzg_recover_each_report* report)
{
    host::KzgRecoverEachShape S;
    char why[320];
    int rc = host::kzg_recover_each_verdict("host kzg_recover_cells_each", cell_offsets, cell, values, n, coset, degree_bound, batch, coeffs_out, stride_elems, report,
                                            &S, why, sizeof why);
    if (rc == BBGPU_OK)
        rc = host::kzg_recover_cells_each_host(S, cell_offsets, cell, values, degree_bound, batch, coeffs_out, stride_elems, values_out, first_bad_out, report, why,
                                               sizeof why);
    if (rc) set_error("%s", why);
    return rc;
}

// `count` transforms of 2^lg elements, `stride` elements apart, through the internal entry: no cap of 64, the grid's limit in y respected, the shared
// scratch sized for a whole chunk (transforms above 2^11 points go through it)
static int recover_each_ntt(uint64_t* d, size_t stride, size_t count, int lg, int kind, hipStream_t st)
{
    constexpr size_t CHUNK = 32768;
    if (lg > 11)
        if (int rc = grow(&ctx().d_scratch, &ctx().scratch_cap, (std::min(count, CHUNK) << lg) * 32)) return rc;
    if (int rc = shared_begin(st)) return rc;
    for (size_t c0 = 0; c0 < count; c0 += CHUNK) {
        const int rc = ntt_device_batch(d + 4 * c0 * stride, stride, (int)std::min(CHUNK, count - c0), ctx().d_scratch, lg, kind, nullptr, st);
        if (rc == BBGPU_ERR_HIP) {
            const hipError_t he = hipGetLastError(); // hipSuccess: the failing call has already described itself (launch_check / dev_malloc)
            if (he != hipSuccess) set_error("NTT launch failed: %s", hipGetErrorString(he));
        }
        if (rc) return rc;
    }
    return shared_end(st);
}

int bbgpu_kzg_recover_cells_each(const uint32_t* cell_offsets, const uint32_t* cell, const uint64_t* values, size_t n, size_t coset, size_t degree_bound, int batch,
                                 uint64_t* d_coeffs_out, size_t stride_elems, uint64_t* values_out, uint64_t* first_bad_out,
                                 bbgpu_kzg_recover_each_report* report, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgRecoverEachShape S;
    char why[320];
    if (int rc = host::kzg_recover_each_verdict("kzg_recover_cells_each", cell_offsets, cell, values, n, coset, degree_bound, batch, d_coeffs_out, stride_elems,
                                                report, &S, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    const size_t m = S.m, total = S.total, B = (size_t)batch;
    const int log2m = S.log2n - S.log2l;
    size_t M = 1; // the common padded number of roots: a power of two, >= every mu_b, <= m (every polynomial lists a cell)
    while (M < S.max_missing) M <<= 1;
    const size_t T = std::min<size_t>(KZG_RECOVER_EACH_LEAF, M);
    StageEvents<6> ev; // the stage boundaries of bbgpu_last_timing
    if (int rc = ev.create(ctx().timing != 0)) return rc;
    // offsets, counts of missing cells, cell lists and padded missing lists in one array | the tree | the inputs of the two Z transforms, then z and z',
    // and the power table | the values | the findings | the copy the forward transform works in
    DevBuf lists, tree, z, vals, find, copy;
    const size_t list_words = (B + 1) + B + total + B * M;
    HIPCHK(dev_malloc(&lists.p, list_words * 4));
    HIPCHK(dev_malloc(&tree.p, B * 2 * M * 32));
    HIPCHK(dev_malloc(&z.p, 2 * B * m * 32 + kzg_recover_each_table_words(log2m) * 4));
    HIPCHK(dev_malloc(&vals.p, total * coset * 32));
    HIPCHK(dev_malloc(&find.p, B * sizeof(RecoverFindings)));
    if (values_out) HIPCHK(dev_malloc(&copy.p, B * n * 32));
    std::vector<uint32_t> all(list_words, ~0u);
    for (size_t b = 0; b <= B; b++) all[b] = cell_offsets[b];
    for (size_t b = 0; b < B; b++) {
        all[B + 1 + b] = (uint32_t)S.missing[b].size();
        std::copy(S.missing[b].begin(), S.missing[b].end(), all.begin() + (2 * B + 1 + total + b * M));
    }
    std::copy(cell, cell + total, all.begin() + (2 * B + 1));
    RecoverLists L{};
    L.d_off = lists.as<uint32_t>();
    L.d_mu = L.d_off + B + 1;
    L.d_cell = L.d_mu + B;
    L.d_missing = L.d_cell + total;
    L.cell_mask = ~0u;
    L.missing_stride = (uint32_t)M;
    L.z_stride = (uint32_t)m;
    uint64_t *d_tree = tree.as<uint64_t>(), *d_z = z.as<uint64_t>(), *d_zc = d_z + 4 * B * m;
    uint32_t* d_tab = reinterpret_cast<uint32_t*>(d_zc + 4 * B * m);
    RecoverFound F(batch);
    if (int rc = host_to_device(lists.p, all.data(), list_words * 4, st)) return rc;
    if (int rc = F.begin(find.p, st)) return rc;
    if (int rc = host_to_device(vals.p, values, total * coset * 32, st)) return rc;
    if (int rc = ev.mark(0, st)) return rc;
    // the tree: leaves of T roots, then one level per doubling -- forward transform of every slot, sibling products, inverse transform of every other slot
    if (int rc = kzg_recover_each_leaves(L.d_missing, batch, M, log2m, d_tree, st)) return rc;
    for (size_t D = T; D < M; D <<= 1) {
        const int lg = log2_exact(2 * D);
        const size_t slots = B * M / D;
        if (int rc = recover_each_ntt(d_tree, 2 * D, slots, lg, BBGPU_FFT, st)) return rc;
        if (int rc = kzg_recover_each_pair(d_tree, slots / 2, lg, st)) return rc;
        if (int rc = recover_each_ntt(d_tree, 4 * D, slots / 2, lg, BBGPU_IFFT, st)) return rc;
    }
    // Z_b's coefficients, scaled for the domain and for the coset, and the 2 x batch transforms of size m that make z and z' x 2^-5 of them
    if (int rc = kzg_recover_each_gather(d_tree, L.d_mu, batch, M, S.log2n, S.log2l, d_tab, d_z, d_zc, st)) return rc;
    if (int rc = recover_each_ntt(d_z, m, 2 * B, log2m, BBGPU_FFT, st)) return rc;
    if (int rc = recover_back_end(L, vals.as<uint64_t>(), d_z, d_zc, B * m, n, S.log2n, S.log2l, degree_bound, batch, d_coeffs_out, stride_elems,
                                  copy.as<uint64_t>(), find.as<RecoverFindings>(), F, ev, hip_stream))
        return rc;
    // the verdict into locals first: nothing of the caller's host memory is written before the last copy has succeeded
    bbgpu_kzg_recover_each_report rep;
    if (int rc = host::kzg_recover_each_report("kzg_recover_cells_each", F.first_bad.data(), F.first_bug.data(), batch, S.max_missing, nullptr, &rep, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (values_out)
        if (int rc = device_to_host_sync(values_out, copy.p, B * n * 32, st)) return rc;
    *report = rep;
    if (first_bad_out) std::copy(F.first_bad.begin(), F.first_bad.end(), first_bad_out);
    return recover_cells_timing(ev, values_out != nullptr);
}

/* ---- transforms and erasure decoding on columns of curve points (host_g1_recover.hpp, g1_recover.hip) ---- */
static int g_g1_stage_mapping = 0; // bbgpu_g1_set_stage_mapping: 0 the dispatch below, 1 and 2 one kernel for every shape (the bench's comparison)
// Which stage kernel runs the transforms of a call: k_g1_stage_cols where a column has fewer butterflies than a wave has lanes (n <= 64) -- the shapes at
// which k_lagrange_stage, one column per blockIdx.y, leaves lanes idle and launches a workgroup per column --, k_lagrange_stage from n = 128 on, where every
// wave of either mapping is full and profiles/g1_recover.txt shows no median lower by more than the legs' full range.
static int g1_transform_dispatch(uint32_t* d_scratch, int log2n, int batch, const host::Fr& root, hipStream_t st)
{
    const Limbs9 r = host::limbs_m261(root);
    const bool cols = g_g1_stage_mapping == 2 || (g_g1_stage_mapping == 0 && log2n <= 6);
    return cols ? g1_cols_transform(d_scratch, log2n, batch, r.d, st) : g1_cols_transform_rows(d_scratch, log2n, batch, r.d, st);
}
int bbgpu_g1_set_stage_mapping(int mapping)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (mapping < 0 || mapping > 2) return BBGPU_ERR_ARG;
    g_g1_stage_mapping = mapping;
    return BBGPU_OK;
}

int bbgpu_host_g1_ntt(const uint64_t* points, uint64_t* points_out, size_t n, int batch, int kind)
{
    char why[320];
    int log2n = 0;
    if (int rc = host::g1_ntt_verdict("host g1_ntt", points, points_out, n, batch, kind, &log2n, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    host::g1_ntt_host(points, points_out, log2n, batch, kind);
    return BBGPU_OK;
}

int bbgpu_g1_ntt(const uint64_t* points, uint64_t* points_out, size_t n, int batch, int kind, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    char why[320];
    int log2n = 0;
    if (int rc = host::g1_ntt_verdict("g1_ntt", points, points_out, n, batch, kind, &log2n, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    const size_t total = (size_t)batch * n;
    // the points, then the affine results | the scratch
    DevBuf io, scratch;
    HIPCHK(dev_malloc(&io.p, total * 64));
    HIPCHK(dev_malloc(&scratch.p, total * 128));
    if (int rc = host_to_device(io.p, points, total * 64, st)) return rc;
    host::Fr winv, ninv;
    host::srs_lagrange_constants(log2n, &winv, &ninv);
    const bool inverse = kind == BBGPU_IFFT;
    if (int rc = g1_cols_load(io.as<uint32_t>(), n, nullptr, nullptr, inverse ? ninv.d : nullptr, scratch.as<uint32_t>(), log2n, batch, st)) return rc;
    if (int rc = g1_transform_dispatch(scratch.as<uint32_t>(), log2n, batch, inverse ? winv : host::fr_root_of_unity(log2n), st)) return rc;
    if (int rc = g1_cols_finish(scratch.as<uint32_t>(), io.as<uint32_t>(), log2n, batch, st)) return rc;
    return device_to_host_sync(points_out, io.p, total * 64, st);
}

int bbgpu_host_g1_recover(const uint32_t* row, size_t count, const uint64_t* points, size_t n, size_t degree_bound, int batch, uint64_t* points_out,
                          bbgpu_g1_recover_report* report)
{
    host::KzgRecoverShape S;
    char why[320];
    int rc = host::g1_recover_verdict("host g1_recover", row, count, points, n, degree_bound, batch, points_out, report, &S, why, sizeof why);
    if (rc == BBGPU_OK) rc = host::g1_recover_host(S, row, count, points, degree_bound, batch, points_out, report, why, sizeof why);
    if (rc) set_error("%s", why);
    return rc;
}

int bbgpu_g1_recover(const uint32_t* row, size_t count, const uint64_t* points, size_t n, size_t degree_bound, int batch, uint64_t* points_out,
                     bbgpu_g1_recover_report* report, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgRecoverShape S;
    char why[320];
    if (int rc = host::g1_recover_verdict("g1_recover", row, count, points, n, degree_bound, batch, points_out, report, &S, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    const size_t mu = S.mu, total = (size_t)batch * n;
    const int lg = S.log2n;
    StageEvents<7> ev; // the stage boundaries of bbgpu_last_timing
    if (int rc = ev.create(ctx().timing != 0)) return rc;
    // the place of every row in the list and the missing rows | z, z', the four scalar tables and the roots of the missing rows | the points | the
    // findings | the two scratches (the first one takes the affine results at the end)
    DevBuf lists, zt, in, find, scratch;
    HIPCHK(dev_malloc(&lists.p, 2 * n * 4));
    HIPCHK(dev_malloc(&zt.p, 6 * n * 32 + mu * sizeof(Limbs9)));
    HIPCHK(dev_malloc(&in.p, (size_t)batch * count * 64));
    HIPCHK(dev_malloc(&find.p, (size_t)batch * sizeof(RecoverFindings)));
    HIPCHK(dev_malloc(&scratch.p, 2 * total * 128));
    uint32_t *d_slot_of = lists.as<uint32_t>(), *d_missing = d_slot_of + n;
    uint64_t *d_z = zt.as<uint64_t>(), *d_zc = d_z + 4 * n, *d_tabs = d_zc + 4 * n;
    const uint64_t *d_kz = d_tabs, *d_kg = d_tabs + 4 * n, *d_kq = d_tabs + 8 * n, *d_kgi = d_tabs + 12 * n;
    uint32_t* d_roots = reinterpret_cast<uint32_t*>(d_tabs + 16 * n);
    uint32_t *A = scratch.as<uint32_t>(), *B = A + total * 32;
    std::vector<uint32_t> both(2 * n, ~0u);
    for (size_t t = 0; t < count; t++) both[row[t]] = (uint32_t)t;
    std::copy(S.missing.begin(), S.missing.end(), both.begin() + (ptrdiff_t)n);
    RecoverFound F(batch);
    if (int rc = host_to_device(lists.p, both.data(), 2 * n * 4, st)) return rc;
    if (int rc = F.begin(find.p, st)) return rc;
    if (int rc = host_to_device(in.p, points, (size_t)batch * count * 64, st)) return rc;
    host::Fr winv, ninv;
    host::srs_lagrange_constants(lg, &winv, &ninv);
    const host::Fr w = host::fr_root_of_unity(lg), g = host::fr_from_limbs(FrHostP::GEN5);
    if (int rc = ev.mark(0, st)) return rc;
    if (int rc = kzg_recover_vanish(d_missing, mu, lg, 0, d_roots, d_z, d_zc, st)) return rc;
    if (int rc = ev.mark(1, st)) return rc;
    if (int rc = bbgpu_fr_batch_invert_device(d_zc, n, hip_stream)) return rc; // z' is never zero: g^n != 1
    if (int rc = g1_cols_scalars(d_z, d_zc, d_tabs, lg, host::limbs_m256(ninv).d, host::limbs_m261(g).d, host::limbs_m261(host::fr_inv(g)).d, st)) return rc;
    if (int rc = ev.mark(2, st)) return rc;
    if (int rc = g1_cols_load(in.as<uint32_t>(), count, d_slot_of, d_kz, nullptr, A, lg, batch, st)) return rc;
    if (int rc = g1_transform_dispatch(A, lg, batch, winv, st)) return rc;
    if (int rc = ev.mark(3, st)) return rc;
    if (int rc = g1_cols_scale(A, B, d_kg, lg, batch, st)) return rc;
    if (int rc = g1_transform_dispatch(B, lg, batch, w, st)) return rc;
    if (int rc = g1_cols_scale(B, A, d_kq, lg, batch, st)) return rc;
    if (int rc = g1_transform_dispatch(A, lg, batch, winv, st)) return rc;
    if (int rc = g1_cols_scale(A, B, d_kgi, lg, batch, st)) return rc;
    if (int rc = g1_cols_verdict(B, lg, batch, degree_bound, count, find.as<RecoverFindings>(), st)) return rc;
    if (int rc = ev.mark(4, st)) return rc;
    if (int rc = g1_transform_dispatch(B, lg, batch, w, st)) return rc;
    if (int rc = ev.mark(6, st)) return rc;
    if (int rc = g1_cols_finish(B, A, lg, batch, st)) return rc;
    if (int rc = ev.mark(5, st)) return rc;
    if (int rc = F.end(find.p, st)) return rc;
    // the verdict into a local first: nothing of the caller's host memory is written before the last copy has succeeded
    bbgpu_g1_recover_report rep;
    if (int rc = host::g1_recover_report_of("g1_recover", F.first_bad.data(), F.first_bug.data(), batch, mu, &rep, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = device_to_host_sync(points_out, A, total * 64, st)) return rc;
    *report = rep;
    if (ev.on) { // bbgpu_last_timing: 0 the vanishing values, 1 load and IFFT, 2 shift, FFT, divide, IFFT, unshift and verdict, 3 the last FFT and the finish,
                 // 4 the finish alone (a part of 3)
        ctx().last.count = 5;
        if (int rc = ev.ms(6, 5, &ctx().last.ms[4])) return rc;
        if (int rc = ev.ms(0, 1, &ctx().last.ms[0])) return rc;
        if (int rc = ev.ms(2, 3, &ctx().last.ms[1])) return rc;
        if (int rc = ev.ms(3, 4, &ctx().last.ms[2])) return rc;
        if (int rc = ev.ms(4, 5, &ctx().last.ms[3])) return rc;
    }
    return BBGPU_OK;
}

/* ---- the same for columns whose row sets differ (host_g1_recover.hpp, g1_recover.hip) ---- */
int bbgpu_host_g1_recover_each(const uint32_t* row_offsets, const uint32_t* row, const uint64_t* points, size_t n, size_t degree_bound, int batch,
                               uint64_t* points_out, uint64_t* first_bad_out, bbgpu_g1_recover_each_report* report)
{
    host::KzgRecoverEachShape S;
    char why[320];
    int rc = host::g1_recover_each_verdict("host g1_recover_each", row_offsets, row, points, n, degree_bound, batch, points_out, report, &S, why, sizeof why);
    if (rc == BBGPU_OK) rc = host::g1_recover_each_host(S, row_offsets, row, points, degree_bound, batch, points_out, first_bad_out, report, why, sizeof why);
    if (rc) set_error("%s", why);
    return rc;
}

int bbgpu_g1_recover_each(const uint32_t* row_offsets, const uint32_t* row, const uint64_t* points, size_t n, size_t degree_bound, int batch,
                          uint64_t* points_out, uint64_t* first_bad_out, bbgpu_g1_recover_each_report* report, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::KzgRecoverEachShape S;
    char why[320];
    if (int rc = host::g1_recover_each_verdict("g1_recover_each", row_offsets, row, points, n, degree_bound, batch, points_out, report, &S, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    const size_t B = (size_t)batch, total = B * n, listed = S.total, gone = total - listed;
    const int lg = S.log2n;
    StageEvents<7> ev; // the stage boundaries of bbgpu_last_timing
    if (int rc = ev.create(ctx().timing != 0)) return rc;
    // per column the place of every row in its list, the row offsets, the offsets of the missing rows and the missing rows of all columns, in one array |
    // z, z' and the tables kz and kq per column, kg and kgi, and the roots | the points | the findings | the two scratches (the first one takes the
    // affine results at the end)
    DevBuf lists, zt, in, find, scratch;
    const size_t list_words = total + 2 * (B + 1) + gone;
    HIPCHK(dev_malloc(&lists.p, list_words * 4));
    HIPCHK(dev_malloc(&zt.p, (4 * B + 2) * n * 32 + n * sizeof(Limbs9)));
    HIPCHK(dev_malloc(&in.p, listed * 64));
    HIPCHK(dev_malloc(&find.p, B * sizeof(RecoverFindings)));
    HIPCHK(dev_malloc(&scratch.p, 2 * total * 128));
    uint32_t *d_slot_of = lists.as<uint32_t>(), *d_off = d_slot_of + total, *d_moff = d_off + (B + 1), *d_missing = d_moff + (B + 1);
    uint64_t *d_z = zt.as<uint64_t>(), *d_zc = d_z + 4 * total, *d_tabs = d_zc + 4 * total;
    const uint64_t *d_kz = d_tabs, *d_kg = d_kz + 4 * total, *d_kq = d_kg + 4 * n, *d_kgi = d_kq + 4 * total;
    uint32_t* d_roots = reinterpret_cast<uint32_t*>(d_tabs + 4 * (2 * total + 2 * n));
    uint32_t *A = scratch.as<uint32_t>(), *Bs = A + total * 32;
    std::vector<uint32_t> all(list_words, ~0u);
    size_t at = 0; // missing rows so far
    for (size_t b = 0; b < B; b++) {
        const uint32_t first = row_offsets[b], count = row_offsets[b + 1] - first;
        for (uint32_t t = 0; t < count; t++) all[b * n + row[first + t]] = t;
        all[total + b] = first;
        all[total + (B + 1) + b] = (uint32_t)at;
        std::copy(S.missing[b].begin(), S.missing[b].end(), all.begin() + (ptrdiff_t)(total + 2 * (B + 1) + at));
        at += S.missing[b].size();
    }
    all[total + B] = row_offsets[B];
    all[total + (B + 1) + B] = (uint32_t)at; // == gone
    RecoverFound F(batch);
    if (int rc = host_to_device(lists.p, all.data(), list_words * 4, st)) return rc;
    if (int rc = F.begin(find.p, st)) return rc;
    if (int rc = host_to_device(in.p, points, listed * 64, st)) return rc;
    host::Fr winv, ninv;
    host::srs_lagrange_constants(lg, &winv, &ninv);
    const host::Fr w = host::fr_root_of_unity(lg), g = host::fr_from_limbs(FrHostP::GEN5);
    if (int rc = ev.mark(0, st)) return rc;
    if (int rc = g1_cols_vanish(d_moff, d_missing, lg, batch, d_roots, d_z, d_zc, st)) return rc;
    if (int rc = ev.mark(1, st)) return rc;
    if (int rc = bbgpu_fr_batch_invert_device(d_zc, total, hip_stream)) return rc; // z' is never zero: g^n != 1
    if (int rc = g1_cols_scalars(d_z, d_zc, d_tabs, lg, host::limbs_m256(ninv).d, host::limbs_m261(g).d, host::limbs_m261(host::fr_inv(g)).d, st, batch)) return rc;
    if (int rc = ev.mark(2, st)) return rc;
    if (int rc = g1_cols_load(in.as<uint32_t>(), 0, d_slot_of, d_kz, nullptr, A, lg, batch, st, d_off)) return rc;
    if (int rc = g1_transform_dispatch(A, lg, batch, winv, st)) return rc;
    if (int rc = ev.mark(3, st)) return rc;
    if (int rc = g1_cols_scale(A, Bs, d_kg, lg, batch, st)) return rc;
    if (int rc = g1_transform_dispatch(Bs, lg, batch, w, st)) return rc;
    if (int rc = g1_cols_scale(Bs, A, d_kq, lg, batch, st, true)) return rc;
    if (int rc = g1_transform_dispatch(A, lg, batch, winv, st)) return rc;
    if (int rc = g1_cols_scale(A, Bs, d_kgi, lg, batch, st)) return rc;
    if (int rc = g1_cols_verdict(Bs, lg, batch, degree_bound, 0, find.as<RecoverFindings>(), st, d_off)) return rc;
    if (int rc = ev.mark(4, st)) return rc;
    if (int rc = g1_transform_dispatch(Bs, lg, batch, w, st)) return rc;
    if (int rc = ev.mark(6, st)) return rc;
    if (int rc = g1_cols_finish(Bs, A, lg, batch, st)) return rc;
    if (int rc = ev.mark(5, st)) return rc;
    if (int rc = F.end(find.p, st)) return rc;
    // the verdict into locals first: nothing of the caller's host memory is written before the last copy has succeeded
    bbgpu_g1_recover_each_report rep;
    if (int rc = host::g1_recover_each_report_of("g1_recover_each", F.first_bad.data(), F.first_bug.data(), batch, S.max_missing, nullptr, &rep, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = device_to_host_sync(points_out, A, total * 64, st)) return rc;
    *report = rep;
    if (first_bad_out) std::copy(F.first_bad.begin(), F.first_bad.end(), first_bad_out);
    if (ev.on) { // bbgpu_last_timing: 0 the roots and the vanishing values, 1 load and IFFT, 2 shift, FFT, divide, IFFT, unshift and verdict, 3 the last FFT and
                 // the finish, 4 the finish alone (a part of 3)
        ctx().last.count = 5;
        if (int rc = ev.ms(6, 5, &ctx().last.ms[4])) return rc;
        if (int rc = ev.ms(0, 1, &ctx().last.ms[0])) return rc;
        if (int rc = ev.ms(2, 3, &ctx().last.ms[1])) return rc;
        if (int rc = ev.ms(3, 4, &ctx().last.ms[2])) return rc;
        if (int rc = ev.ms(4, 5, &ctx().last.ms[3])) return rc;
    }
    return BBGPU_OK;
}

/* ---- transforms and the erasure decoder down the columns of a resident matrix (host_fr_columns.hpp, fr_columns.hip) ---- */
int bbgpu_host_fr_ntt_columns(uint64_t* rows_mem, size_t rows, size_t width, size_t stride_elems, int kind)
{
    int lg;
    char why[320];
    if (int rc = host::fr_ntt_columns_verdict("host fr_ntt_columns", rows_mem, rows, width, stride_elems, kind, &lg, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    host::fr_ntt_columns_host(rows_mem, lg, width, stride_elems, kind);
    return BBGPU_OK;
}

int bbgpu_fr_ntt_columns_device(uint64_t* d_rows, size_t rows, size_t width, size_t stride_elems, int kind, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    int lg;
    char why[320];
    if (int rc = host::fr_ntt_columns_verdict("fr_ntt_columns", d_rows, rows, width, stride_elems, kind, &lg, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    DevBuf tabs; // the twiddles (the shift tables beside them are not read)
    HIPCHK(dev_malloc(&tabs.p, fr_cols_table_words(lg, 0) * 4));
    if (int rc = fr_cols_tables(nullptr, nullptr, 0, lg, tabs.as<uint32_t>(), st)) return rc;
    if (int rc = fr_cols_transform(d_rows, width, stride_elems, lg, kind == BBGPU_IFFT, tabs.as<uint32_t>(), st)) return rc;
    HIPCHK(hipStreamSynchronize(st)); // the tables go when this returns
    return BBGPU_OK;
}

int bbgpu_host_fr_recover_columns(const uint32_t* set_offsets, const uint32_t* row, int sets, uint64_t* rows_mem, size_t rows, size_t width, size_t stride_elems,
                                  size_t degree_bound, uint32_t* first_bad_out, bbgpu_fr_recover_columns_report* report)
{
    host::FrColumnsShape S;
    char why[320];
    int rc = host::fr_recover_columns_verdict("host fr_recover_columns", set_offsets, row, sets, rows_mem, rows, width, stride_elems, degree_bound, report, &S, why,
                                              sizeof why);
    if (rc == BBGPU_OK) rc = host::fr_recover_columns_host(S, set_offsets, row, rows_mem, degree_bound, first_bad_out, report, why, sizeof why);
    if (rc) set_error("%s", why);
    return rc;
}

int bbgpu_fr_recover_columns_device(const uint32_t* set_offsets, const uint32_t* row, int sets, uint64_t* d_rows, size_t rows, size_t width, size_t stride_elems,
                                    size_t degree_bound, uint32_t* first_bad_out, bbgpu_fr_recover_columns_report* report, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    // argument errors before a device is bound
    host::FrColumnsShape S;
    char why[320];
    if (int rc = host::fr_recover_columns_verdict("fr_recover_columns", set_offsets, row, sets, d_rows, rows, width, stride_elems, degree_bound, report, &S, why,
                                                  sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    if (int rc = ensure_init()) return rc;
    const hipStream_t st = (hipStream_t)hip_stream;
    const int lg = S.log2rows;
    const size_t entries = (size_t)sets * rows, gone = S.missing.size(), mask_words = (entries + 31) / 32;
    StageEvents<3> ev; // the stage boundaries of bbgpu_last_timing
    if (int rc = ev.create(ctx().timing != 0)) return rc;
    // the offsets of the missing rows, the missing rows of all sets and the bits of the present ones, in one array | z, z', the tables and the roots | the
    // call's two findings | every column's finding, if the caller wants them
    DevBuf lists, zt, find, bad;
    const size_t list_words = (size_t)sets + 1 + gone + mask_words, tab_words = fr_cols_table_words(lg, entries);
    HIPCHK(dev_malloc(&lists.p, list_words * 4));
    HIPCHK(dev_malloc(&zt.p, 2 * entries * 32 + tab_words * 4 + rows * sizeof(Limbs9)));
    HIPCHK(dev_malloc(&find.p, 2 * sizeof(unsigned long long)));
    if (first_bad_out) HIPCHK(dev_malloc(&bad.p, width * 4));
    uint32_t *d_moff = lists.as<uint32_t>(), *d_missing = d_moff + sets + 1, *d_present = d_missing + gone;
    uint64_t *d_z = zt.as<uint64_t>(), *d_zc = d_z + 4 * entries;
    uint32_t *d_tabs = reinterpret_cast<uint32_t*>(d_zc + 4 * entries), *d_roots = d_tabs + tab_words;
    std::vector<uint32_t> all(list_words, 0);
    std::copy(S.moff.begin(), S.moff.end(), all.begin());
    std::copy(S.missing.begin(), S.missing.end(), all.begin() + sets + 1);
    for (int s = 0; s < sets; s++)
        for (uint32_t t = set_offsets[s]; t < set_offsets[s + 1]; t++) {
            const size_t bit = (size_t)s * rows + row[t];
            all[(size_t)sets + 1 + gone + bit / 32] |= 1u << (bit % 32);
        }
    unsigned long long keys[2] = { ~0ull, ~0ull };
    if (int rc = host_to_device(lists.p, all.data(), list_words * 4, st)) return rc;
    if (int rc = host_to_device(find.p, keys, sizeof keys, st)) return rc;
    if (int rc = ev.mark(0, st)) return rc;
    if (int rc = g1_cols_vanish(d_moff, d_missing, lg, sets, d_roots, d_z, d_zc, st)) return rc;
    if (int rc = bbgpu_fr_batch_invert_device(d_zc, entries, hip_stream)) return rc; // z' is never zero: g^rows != 1
    if (int rc = fr_cols_tables(d_z, d_zc, entries, lg, d_tabs, st)) return rc;
    if (int rc = ev.mark(1, st)) return rc;
    if (int rc = fr_cols_decode(d_rows, width, stride_elems, lg, sets, degree_bound, d_tabs, d_moff, d_present, bad.as<uint32_t>(), find.as<unsigned long long>(), st))
        return rc;
    if (int rc = ev.mark(2, st)) return rc;
    if (int rc = device_to_host_sync(keys, find.p, sizeof keys, st)) return rc;
    // the verdict into locals first: nothing of the caller's host memory is written before the last copy has succeeded
    bbgpu_fr_recover_columns_report rep;
    const size_t bad_column = keys[0] == ~0ull ? width : (size_t)(keys[0] >> 32), bug_column = keys[1] == ~0ull ? width : (size_t)(keys[1] >> 32);
    if (int rc = host::fr_recover_columns_report_of("fr_recover_columns", width, bad_column, keys[0] & 0xffffffffull, bug_column, keys[1] & 0xffffffffull,
                                                    S.max_missing, &rep, why, sizeof why)) {
        set_error("%s", why);
        return rc;
    }
    std::vector<uint32_t> per_column;
    if (first_bad_out) {
        per_column.resize(width);
        if (int rc = device_to_host_sync(per_column.data(), bad.p, width * 4, st)) return rc;
    }
    if (ev.on) { // bbgpu_last_timing: 0 the roots, the vanishing values, their inversion and the tables, 1 the decode kernel
        float ms[2];
        if (int rc = ev.ms(0, 1, &ms[0])) return rc;
        if (int rc = ev.ms(1, 2, &ms[1])) return rc;
        ctx().last.count = 2;
        ctx().last.ms[0] = ms[0];
        ctx().last.ms[1] = ms[1];
    }
    *report = rep;
    if (first_bad_out) std::copy(per_column.begin(), per_column.end(), first_bad_out);
    return BBGPU_OK;
}

int bbgpu_srs_has_window_tables(int srs_handle)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (srs_handle < 0 || srs_handle >= (int)ctx().srs.size() || !ctx().srs[srs_handle].live) return BBGPU_ERR_ARG;
    return ctx().srs[srs_handle].has_tab() ? 1 : 0;
}

int bbgpu_msm_g1_device_rows_async(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, uint64_t row_begin, uint64_t row_end,
                                   void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const SrsEntry* ep = nullptr;
    if (int rc = share_ticket_srs(srs_handle, offset, d_scalars, n, "row", &ep)) return rc;
    const SrsEntry& e = *ep;
    int t;
    hipStream_t st;
    if (int rc = begin_ticket(hip_stream, &t, &st)) return rc;
    if (n && row_end > row_begin && !windows_resident(e, (int)(row_begin / n), (int)((row_end + n - 1) / n))) return BBGPU_ERR_STATE;
    const int rc = msm_issue_rows(ctx().slot[t], e.d_srs + offset * 16, e.segs[0].d_tab + offset * 16, e.n, e.tab_c, d_scalars, n, row_begin, row_end, st, ctx().timing);
    if (rc == BBGPU_ERR_ARG) set_error("bad row range [%llu, %llu) of %d x %zu", (unsigned long long)row_begin, (unsigned long long)row_end, e.tab_W, n);
    return rc ? rc : commit_ticket(t);
}

int bbgpu_msm_g1_device_buckets_async(int srs_handle, size_t offset, const uint64_t* d_scalars, size_t n, int share, int share_count, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const SrsEntry* ep = nullptr;
    if (int rc = share_ticket_srs(srs_handle, offset, d_scalars, n, "bucket", &ep)) return rc;
    const SrsEntry& e = *ep;
    int t;
    hipStream_t st;
    if (int rc = begin_ticket(hip_stream, &t, &st)) return rc;
    if (!windows_resident(e, 0, e.tab_W)) return BBGPU_ERR_STATE; // every share reads every window's table
    if (share < 0 || share_count < 1 || share >= share_count) {
        set_error("bad bucket share %d of %d", share, share_count);
        return BBGPU_ERR_ARG;
    }
    const int rc = msm_issue_buckets(ctx().slot[t], e.d_srs + offset * 16, e.segs[0].d_tab + offset * 16, e.n, e.tab_c, d_scalars, n, (uint32_t)share, (uint32_t)share_count, st, ctx().timing);
    if (rc == BBGPU_ERR_ARG) set_error("bad bucket share %d of %d (at most one share per row of the bucket matrix)", share, share_count);
    return rc ? rc : commit_ticket(t);
}

int bbgpu_msm_g1_device_batch_async(int srs_handle, size_t offset, const uint64_t* const* d_scalars, int jobs, size_t n, void* hip_stream)
{
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    const SrsEntry* ep = nullptr;
    if (int rc = ticket_srs(srs_handle, &ep)) return rc;
    const SrsEntry& e = *ep;
    if (!d_scalars || jobs < 1 || offset + n > e.n) {
        set_error("bad batch: jobs %d, range [%zu, %zu) of %zu points", jobs, offset, offset + n, e.n);
        return BBGPU_ERR_ARG;
    }
    if ((!e.has_tab() && jobs > 1) || jobs > MSM_MAX_JOBS) {
        set_error("batched MSM: 1..%d jobs over an SRS registered with window tables (bbgpu_set_precompute, n >= 1024)", MSM_MAX_JOBS);
        return BBGPU_ERR_ARG;
    }
    int t;
    hipStream_t st;
    if (int rc = begin_ticket(hip_stream, &t, &st)) return rc;
    const int rc = issue_ticket(t, e, offset, d_scalars, jobs, n, 0, entry_windows(e, n), st);
    return rc ? rc : commit_ticket(t);
}

// The blocking part of a wait runs WITHOUT the library mutex: the events of the ticket's slot (and of its helper) are picked up under the lock,
// waited for outside it, and only the host finish -- which then finds them complete -- takes the lock again.  A thread that collects tickets
// therefore never stops another one from issuing (a rank of a multi-GPU split issues from one thread and collects / exchanges on another,
// barretenberg_amd/sharding.py; the reference calls pippenger() from an OpenMP region).  The caller's part of the contract is the usual one: a
// ticket is waited for once, by one thread.
static void wait_ticket_events_unlocked(int ticket)
{
    hipEvent_t ev[2] = { nullptr, nullptr };
    {
        std::lock_guard<std::recursive_mutex> lk(g_mu);
        if (ticket < 0 || ticket >= Context::NSLOT || !ctx().slot[ticket].pending || ctx().slot[ticket].is_helper) return; // the locked part reports it
        const MsmSlot& S = ctx().slot[ticket];
        ev[0] = S.done;
        if (S.helper >= 0) ev[1] = ctx().slot[S.helper].done;
    }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventSynchronize(e); // errors surface in the locked finish, which synchronises again
}

int bbgpu_msm_g1_batch_wait(int ticket, uint64_t* out)
{
    wait_ticket_events_unlocked(ticket);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (ticket < 0 || ticket >= Context::NSLOT || !ctx().slot[ticket].pending || ctx().slot[ticket].is_helper || !out) {
        set_error("no MSM batch in flight for ticket %d", ticket);
        return BBGPU_ERR_ARG;
    }
    host::Xyzz res[MSM_MAX_JOBS];
    const uint32_t jobs = ctx().slot[ticket].jobs;
    int rc = finish_ticket(ticket, res, &ctx().last);
    if (rc) return rc;
    host::g1_batch_to_normalised(res, jobs, out); // one inversion for the whole batch
    return BBGPU_OK;
}

int bbgpu_msm_g1_wait(int ticket, uint64_t out[12])
{
    wait_ticket_events_unlocked(ticket);
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    if (ticket < 0 || ticket >= Context::NSLOT || !ctx().slot[ticket].pending || ctx().slot[ticket].is_helper || ctx().slot[ticket].jobs != 1) {
        set_error("no MSM in flight for ticket %d", ticket);
        return BBGPU_ERR_ARG;
    }
    host::Xyzz res;
    int rc = finish_ticket(ticket, &res, &ctx().last);
    if (rc) return rc;
    host::g1_to_normalised(res, out);
    return BBGPU_OK;
}

int bbgpu_g1_sum(const uint64_t* points12, size_t count, uint64_t out[12])
{
    if (!out || (count && !points12)) return BBGPU_ERR_ARG;
    host::Xyzz acc = host::g1_infinity();
    for (size_t i = 0; i < count; i++) acc = host::g1_add(acc, host::g1_from_jacobian(points12 + 12 * i));
    host::g1_to_normalised(acc, out);
    return BBGPU_OK;
}

} // extern "C"
#pragma GCC visibility pop
