// plonk.hip -- the PLONK prover rounds with every polynomial resident in HBM (BASELINE config 5).
//
// Restates waffle::Prover::construct_proof (src/barretenberg/waffle/proof_system/prover/prover.cpp:661-670) for the
// standard arithmetic circuit (widgets/arithmetic_widget.cpp) and its optional widgets: the rounds below cite the lines they
// follow.  The reference moves every polynomial across the boundary for each of its 26 transforms and
// 9 commitments; here the witness and circuit polynomials are uploaded once, all NTTs (ntt.hip), MSMs (msm.hip) and the
// O(n) loops in between (poly.hip) run on the device, and only 32-byte evaluations and 96-byte commitments come back --
// they have to, because the Fiat-Shamir challenges (challenge.hpp:64-135, Keccak-256 on the host) depend on them.
//
// There is ONE prover: PlonkProver::prove() advances the five rounds in lockstep over the lanes of a lane set.  A single proof
// (bbgpu_plonk_construct_proof) is that engine over the handle's own lane, whose wires are the witness the handle holds; a
// batch (bbgpu_plonk_construct_proof_batch*) is the same engine over the batch lanes, loaded from the caller's witnesses first.
// Witness loading (load_lanes) and the witness check (check_enqueue / check_finish) address the current set in the same way.
// Either kind of call flushes its kernels' table records through h2d_async and reads its result slots through d2h_async, so
// both pass the h2d / d2h fault funnels (bbgpu_fault_inject).
//
// Bit-exactness: every proof element is a canonical field value or a normalised curve point, both unique, and exact
// arithmetic makes them independent of evaluation order; the proof bytes equal the reference's (tests/golden/plonk_proofs.json).
// State that depends only on the circuit (sigma polynomials, selector transforms) or only on n (subgroup table, L_1 on the
// 2n coset) is computed on first use and kept, where the reference recomputes it inside every construct_proof().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "bbgpu_internal.h"
#include "host_fr.hpp"
#include "host_g1.hpp"
#include "host_plonk_check.hpp"
#include "keccak.hpp"
#include "poly.h"

namespace bbgpu {
namespace {

using host::Fr;

#define RC(x)                                                                                                          \
    do {                                                                                                               \
        int rc_ = (x);                                                                                                 \
        if (rc_) return rc_;                                                                                           \
    } while (0)

int ilog2(size_t n)
{
    int l = 0;
    while (((size_t)1 << l) < n) l++;
    return l;
}
double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// waffle_types.hpp:18-45, the part the standard arithmetic circuit fills: 9 commitments (x, y) then 7 evaluations
struct Proof {
    uint64_t W_L[8], W_R[8], W_O[8], Z_1[8], T_LO[8], T_MID[8], T_HI[8], PI_Z[8], PI_Z_OMEGA[8];
    Fr w_l_eval, w_r_eval, w_o_eval, sigma_1_eval, sigma_2_eval, z_1_shifted_eval, linear_eval;
    Fr w_l_shifted_eval, w_r_shifted_eval, w_o_shifted_eval, q_c_eval, q_mimc_coefficient_eval; // widget-dependent (waffle_types.hpp:39-43)
};
static_assert(sizeof(Proof) == BBGPU_PLONK_PROOF_WORDS * 8, "proof layout");

struct Challenges {
    Fr beta, gamma, alpha, z, nu;
};

std::atomic<uint64_t> g_lane_bytes{ 0 }; // device bytes held by the lanes of every prover's batches (bbgpu_memory_stats: staging_bytes)

// The streams of a destroyed prover wait here for the next one (under g_pmu, until plonk_release_all_locked).  Events of the library's shared state --
// the staging ring's, the transforms' scratch, the MSM slots' -- were last recorded on them, and the runtime reaches through such an event to the stream
// it was recorded on when the event is waited for (with the streams destroyed per handle: a sporadic "event last recorded in a capturing stream" from
// hipEventSynchronize, in a process that captures nothing).
std::vector<hipStream_t> g_idle_streams;
int take_stream(hipStream_t* s)
{
    if (g_idle_streams.empty()) {
        HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    } else {
        *s = g_idle_streams.back();
        g_idle_streams.pop_back();
    }
    return BBGPU_OK;
}
void give_stream(hipStream_t& s)
{
    if (s) g_idle_streams.push_back(s);
    s = nullptr;
}

class PlonkProver {
  public:
    size_t n = 0;
    int log2n = 0;
    int srs = -1;
    hipStream_t st = nullptr;
    hipStream_t st_ticket[8] = {};  // the commitments' own queues, one per MSM slot (tickets that share a stream serialise), ordered after `st` by an event
    hipEvent_t scalars_ready = nullptr;
    poly::Scratch scratch;          // scans and evaluations of the lanes, the inversion behind L_1
    std::vector<void*> allocs;

    // inputs (prover.hpp:44-59, arithmetic_widget.hpp:45-49): permutation mappings / Lagrange-base selector values
    uint32_t* sigma_mapping[3] = {};
    uint64_t* q_lagrange[5] = {};
    // circuit- / domain-only state, built on first use
    bool circuit_ready = false;
    uint64_t* roots = nullptr;        // w^i, i < n
    uint64_t* sigma_lagrange[3] = {}; // permutation.hpp:15-87
    uint64_t* sigma_coeff = nullptr;  // the three sigma polynomials in coefficient form, UNSCALED (prover.cpp:245-247 without the beta: the lanes scale them by theirs)
    uint64_t* q_coeff[5] = {};        // selector polynomials, coefficient form
    uint64_t* q_fft2n[5] = {};        // their coset evaluations on the 2n domain (unscaled)
    uint64_t* l_1 = nullptr;          // L_1 on the 2n coset
    // optional bool widget (bool_widget.hpp): q_bl, q_br, q_bo
    bool has_bool = false;
    uint64_t* qb_lagrange[3] = {};
    uint64_t* qb_coeff[3] = {};
    uint64_t* qb_fft2n[3] = {};
    // optional MiMC widget (mimc_widget.hpp): [0] = q_mimc_selector, [1] = q_mimc_coefficient
    bool has_mimc = false;
    uint64_t* qm_lagrange[2] = {};
    uint64_t* qm_coeff[2] = {};
    uint64_t* qm_fft4n[2] = {};
    // optional sequential widget (sequential_widget.hpp): q_o_next
    bool has_seq = false;
    uint64_t *qs_lagrange = nullptr, *qs_coeff = nullptr, *qs_fft2n = nullptr;

    // ---- lanes ------------------------------------------------------------------------------------------------------------------------------------------
    // Every proof runs in a LANE: the per-proof vectors, lane-major inside one allocation per group, so that the same polynomial of all lanes of a set is
    // one strided batch for the transforms and one launch (grid.y = lane) for the kernels of poly.hip.  The handle's OWN set has one lane, made with the
    // handle: its G_WLAG group is the witness the handle holds, and bbgpu_plonk_construct_proof proves it.  The BATCH set grows with the largest batch
    // (ensure_lanes) and is counted in g_lane_bytes.  The rounds (prove) and the witness loading and checking address whichever set is current.
    enum {
        G_WLAG,  // wires, Lagrange base                                            (Prover::w_l, w_r, w_o before :130-132)
        G_W,     // wire polynomials, coefficient form                              (after :130-132)
        G_SIGMA, // beta * sigma_i, coefficient form                                (after :245-247)
        G_WFFT,  // the wires on the 4n coset                                       (circuit_state.w_*_fft)
        G_SFFT,  // w_i + beta sigma_i + gamma on the 4n coset
        G_Z,     // grand product polynomial, coefficient form                      (after :221)
        G_ZFFT,  // alpha * Z on the 4n coset
        G_QL,    // quotient_large, 4n
        G_QM,    // quotient_mid, 2n
        G_R,     // linearisation polynomial
        G_TMP,   // workspaces (num / den / opening polynomials)
        G_COUNT
    };
    static constexpr int lane_group_vectors[G_COUNT] = { 3, 3, 3, 12, 12, 1, 4, 4, 2, 1, 3 }; // n-sized vectors per lane: 48 in all
    struct LaneSet {
        int count = 0;                 // lanes it has room for
        uint64_t* group[G_COUNT] = {};
        uint64_t* slots = nullptr;     // 16 x 32 bytes of device results per lane
        uint64_t* vars = nullptr;      // where host variables land before the expansion, num_variables x 32 bytes per lane: made on first use, counted in g_lane_bytes
        size_t vars_bytes = 0;
    };
    struct Lane {
        Challenges ch;
        Proof proof;
        Fr t_eval, beta_inv;
    };
    LaneSet own, batch;
    LaneSet* cur = &own;
    poly::LaneTable lane_tab;
    void* h_lane_slots = nullptr; // pinned mirror of a set's slots, BBGPU_PLONK_MAX_BATCH lanes
    std::vector<Lane> lanes;      // the host side of the lanes of the run in progress

    // what the last single proof / the last batch left for the bbgpu_plonk_last_* / bbgpu_plonk_batch_* getters: neither kind of run writes the other's
    Challenges challenges;
    double timing[8] = {}; // total, msm, ntt+pointwise (the rest), first-use preparation
    Challenges batch_challenges[BBGPU_PLONK_MAX_BATCH] = {};
    int batch_count = 0;
    double batch_timing[4] = {};

    // witness check (bbgpu_plonk_check_witness*, bbgpu_plonk_set_witness_check): the result records of BBGPU_PLONK_MAX_BATCH lanes -- counts, then the
    // atomicMin words (poly.h) -- in one small allocation, made on the first check
    bool witness_check = false;
    poly::WitnessCheckCounts* check_counts = nullptr;
    poly::WitnessCheckFirst* check_first = nullptr;
    void* h_check = nullptr; // pinned mirror
    bbgpu_plonk_witness_report reports[BBGPU_PLONK_MAX_BATCH] = {};
    int report_count = 0;
    static constexpr size_t check_bytes = BBGPU_PLONK_MAX_BATCH * (sizeof(poly::WitnessCheckCounts) + sizeof(poly::WitnessCheckFirst));

    // witnesses as composer variables (bbgpu_plonk_prover_set_wire_map, the VARIABLES form of bbgpu_plonk_witness): the circuit's wire -> variable indices,
    // w_l | w_r | w_o in one allocation.  It and the sets' variables staging are counted with the lanes (g_lane_bytes) and go with the handle.
    uint32_t* wire_map = nullptr;
    size_t num_variables = 0;
    hipEvent_t caller_ready = nullptr; // orders `st` behind the stream a caller produced its device buffers on

    ~PlonkProver() { release(); }
    void release_vars(LaneSet& s)
    {
        if (s.vars) (void)dev_free(s.vars);
        s.vars = nullptr;
        g_lane_bytes -= s.vars_bytes;
        s.vars_bytes = 0;
    }
    void release_wire_map()
    {
        if (wire_map) {
            (void)dev_free(wire_map);
            g_lane_bytes -= 3 * n * 4;
        }
        wire_map = nullptr;
        release_vars(own);
        release_vars(batch);
        num_variables = 0;
    }
    void release()
    {
        if (st) (void)hipStreamSynchronize(st);
        release_lanes();
        release_wire_map();
        if (caller_ready) (void)hipEventDestroy(caller_ready);
        caller_ready = nullptr;
        lane_tab.release();
        if (h_lane_slots) (void)hipHostFree(h_lane_slots);
        h_lane_slots = nullptr;
        for (hipStream_t& q : st_ticket) give_stream(q);
        for (void* p : allocs) (void)dev_free(p); // the circuit's state, the own lane, the check records
        allocs.clear();
        own = LaneSet{};
        if (h_check) (void)hipHostFree(h_check);
        h_check = nullptr;
        check_counts = nullptr;
        check_first = nullptr;
        scratch.release();
        give_stream(st);
        if (scalars_ready) (void)hipEventDestroy(scalars_ready);
        scalars_ready = nullptr;
    }
    template <class T> int dalloc(T** p, size_t bytes)
    {
        HIPCHK(dev_malloc((void**)p, bytes));
        allocs.push_back(*p);
        return BBGPU_OK;
    }

    int init(const bbgpu_plonk_circuit* c, int srs_handle)
    {
        n = c->n;
        log2n = ilog2(n);
        srs = srs_handle;
        RC(take_stream(&st));
        for (hipStream_t& q : st_ticket) RC(take_stream(&q));
        HIPCHK(hipEventCreateWithFlags(&scalars_ready, hipEventDisableTiming));
        const size_t fb = n * 32;
        const uint64_t* hw[3] = { c->w_l, c->w_r, c->w_o };
        const uint32_t* hm[3] = { c->sigma_1_mapping, c->sigma_2_mapping, c->sigma_3_mapping };
        const uint64_t* hq[5] = { c->q_m, c->q_l, c->q_r, c->q_o, c->q_c };
        // the own lane, and what every run needs beside its lanes: nothing of it is made lazily, so that a witness upload allocates its staging only
        own.count = 1;
        for (int g = 0; g < G_COUNT; g++) RC(dalloc(&own.group[g], lane_group_vectors[g] * fb));
        RC(dalloc(&own.slots, 16 * 32));
        HIPCHK(hipHostMalloc(&h_lane_slots, (size_t)BBGPU_PLONK_MAX_BATCH * 16 * 32));
        RC(lane_tab.init((size_t)2 << 20));
        RC(scratch.ensure(std::max(2 * poly::scan_scratch_bytes(n), (size_t)9 * 256 * 32) + 64)); // one lane's two scans / nine evaluations; batches grow it
        // the three sigma polynomials (and the five selectors) sit back to back so that their transforms run as one batched launch
        // (bbgpu_ntt_device_batch): at these sizes a single transform leaves most of the chip idle
        RC(dalloc(&sigma_lagrange[0], 3 * fb));
        RC(dalloc(&sigma_coeff, 3 * fb));
        for (int k = 0; k < 3; k++) {
            sigma_lagrange[k] = sigma_lagrange[0] + (size_t)k * n * 4;
            RC(dalloc(&sigma_mapping[k], n * 4));
            RC(host_to_device(lv(G_WLAG, 0, k), hw[k], fb, st));
            RC(host_to_device(sigma_mapping[k], hm[k], n * 4, st));
        }
        RC(dalloc(&q_lagrange[0], 5 * fb));
        RC(dalloc(&q_coeff[0], 5 * fb));
        RC(dalloc(&q_fft2n[0], 10 * fb));
        for (int k = 0; k < 5; k++) {
            q_lagrange[k] = q_lagrange[0] + (size_t)k * n * 4;
            q_coeff[k] = q_coeff[0] + (size_t)k * n * 4;
            q_fft2n[k] = q_fft2n[0] + (size_t)k * 2 * n * 4;
            RC(host_to_device(q_lagrange[k], hq[k], fb, st));
        }
        const uint64_t* hb[3] = { c->q_bl, c->q_br, c->q_bo };
        has_bool = hb[0] != nullptr;
        if (has_bool) {
            RC(dalloc(&qb_lagrange[0], 3 * fb));
            RC(dalloc(&qb_coeff[0], 3 * fb));
            RC(dalloc(&qb_fft2n[0], 6 * fb));
            for (int k = 0; k < 3; k++) {
                qb_lagrange[k] = qb_lagrange[0] + (size_t)k * n * 4;
                qb_coeff[k] = qb_coeff[0] + (size_t)k * n * 4;
                qb_fft2n[k] = qb_fft2n[0] + (size_t)k * 2 * n * 4;
                RC(host_to_device(qb_lagrange[k], hb[k], fb, st));
            }
        }
        const uint64_t* hmm[2] = { c->q_mimc_selector, c->q_mimc_coefficient };
        has_mimc = hmm[0] != nullptr;
        if (has_mimc) {
            RC(dalloc(&qm_lagrange[0], 2 * fb));
            RC(dalloc(&qm_coeff[0], 2 * fb));
            RC(dalloc(&qm_fft4n[0], 8 * fb));
            for (int k = 0; k < 2; k++) {
                qm_lagrange[k] = qm_lagrange[0] + (size_t)k * n * 4;
                qm_coeff[k] = qm_coeff[0] + (size_t)k * n * 4;
                qm_fft4n[k] = qm_fft4n[0] + (size_t)k * 4 * n * 4;
                RC(host_to_device(qm_lagrange[k], hmm[k], fb, st));
            }
        }
        has_seq = c->q_o_next != nullptr;
        if (has_seq) {
            RC(dalloc(&qs_lagrange, fb));
            RC(dalloc(&qs_coeff, fb));
            RC(dalloc(&qs_fft2n, 2 * fb));
            RC(host_to_device(qs_lagrange, c->q_o_next, fb, st));
        }
        RC(dalloc(&roots, fb));
        RC(dalloc(&l_1, 2 * fb));
        HIPCHK(hipStreamSynchronize(st)); // the caller's arrays may go away after this call (uploads above 8 MiB read them asynchronously)
        return BBGPU_OK;
    }

    // ---- witnesses in other forms and places (bbgpu_plonk_witness) ------------------------------------------------------------------
    int set_wire_map(const uint32_t* const idx[3], size_t nv)
    {
        HIPCHK(hipStreamSynchronize(st));
        release_wire_map(); // the staging is sized by the number of variables: a new map starts over
        uint32_t* d = nullptr;
        HIPCHK(dev_malloc((void**)&d, 3 * n * 4));
        std::vector<uint32_t> all(3 * n);
        for (int k = 0; k < 3; k++) memcpy(all.data() + (size_t)k * n, idx[k], n * 4);
        int rc = host_to_device(d, all.data(), 3 * n * 4, st);
        if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = BBGPU_ERR_HIP; // `all` goes away
        if (rc) {
            (void)hipStreamSynchronize(st);
            (void)dev_free(d);
            return rc;
        }
        wire_map = d;
        num_variables = nv;
        g_lane_bytes += 3 * n * 4;
        return BBGPU_OK;
    }
    // `st` continues behind everything enqueued so far on the stream the caller produced a device buffer on
    int wait_for_caller(void* hip_stream)
    {
        if (!caller_ready) HIPCHK(hipEventCreateWithFlags(&caller_ready, hipEventDisableTiming));
        HIPCHK(hipEventRecord(caller_ready, static_cast<hipStream_t>(hip_stream)));
        HIPCHK(hipStreamWaitEvent(st, caller_ready, 0));
        return BBGPU_OK;
    }
    poly::ExpandWiresArgs expand_args(const uint64_t* variables, uint64_t* const dst[3]) const
    {
        poly::ExpandWiresArgs A{};
        A.variables = (const uint32_t*)variables;
        for (int k = 0; k < 3; k++) {
            A.index[k] = wire_map + (size_t)k * n;
            A.dst[k] = (uint32_t*)dst[k];
        }
        A.n = (uint32_t)n;
        A.num_variables = (uint32_t)num_variables;
        return A;
    }
    // the witness the handle holds, from any form and place (the descriptor has passed check_witness_desc and, for DEVICE, check_device_pointers)
    int set_witness_from(const bbgpu_plonk_witness& W)
    {
        use(own);
        RC(load_lanes(1, &W));
        HIPCHK(hipStreamSynchronize(st)); // the caller's buffers may be reused after this call
        return BBGPU_OK;
    }

    // ---- small helpers ----------------------------------------------------------------------------------------------
    int copy(uint64_t* dst, const uint64_t* src, size_t count)
    {
        HIPCHK(hipMemcpyAsync(dst, src, count * 32, hipMemcpyDeviceToDevice, st));
        return BBGPU_OK;
    }
    // challenge.hpp:15-62: commitments / evaluations enter the transcript out of Montgomery form
    static void put_point(std::vector<uint64_t>& buf, const uint64_t p[8])
    {
        host::Fq x, y, one = { { 1, 0, 0, 0 } };
        memcpy(x.d, p, 32);
        memcpy(y.d, p + 4, 32);
        x = host::fq_mul(x, one);
        y = host::fq_mul(y, one);
        buf.insert(buf.end(), x.d, x.d + 4);
        buf.insert(buf.end(), y.d, y.d + 4);
    }
    static void put_fr(std::vector<uint64_t>& buf, const Fr& v)
    {
        Fr p = host::fr_from_mont(v);
        buf.insert(buf.end(), p.d, p.d + 4);
    }
    static Fr challenge(const std::vector<uint64_t>& buf)
    {
        Fr h;
        host::hash_field_elements(buf.data(), buf.size() / 4, h.d);
        return host::fr_to_mont(h); // challenge.hpp:70-71: the raw 256-bit digest, reduced by the Montgomery conversion
    }
    static std::vector<uint64_t> transcript_of(const Proof& proof, int stage)
    {
        std::vector<uint64_t> b;
        put_point(b, proof.W_L); put_point(b, proof.W_R); put_point(b, proof.W_O);                  // add_wire_commitments_to_buffer
        if (stage >= 1) put_point(b, proof.Z_1);                                                     // add_grand_product_commitments_to_buffer
        if (stage >= 2) { put_point(b, proof.T_LO); put_point(b, proof.T_MID); put_point(b, proof.T_HI); } // add_quotient_commitment_to_buffer
        return b;
    }

    // ---- witness check ----------------------------------------------------------------------------------------------------
    // Needs nothing that a proof computes: the wire values as uploaded, the selector VALUES and the mappings of init().
    int ensure_check()
    {
        if (check_counts) return BBGPU_OK;
        if (!h_check) HIPCHK(hipHostMalloc(&h_check, check_bytes));
        uint8_t* d = nullptr;
        RC(dalloc(&d, check_bytes));
        check_counts = reinterpret_cast<poly::WitnessCheckCounts*>(d);
        check_first = reinterpret_cast<poly::WitnessCheckFirst*>(d + BBGPU_PLONK_MAX_BATCH * sizeof(poly::WitnessCheckCounts));
        return BBGPU_OK;
    }
    poly::WitnessCheckArgs check_args(int lane) const
    {
        poly::WitnessCheckArgs A{};
        A.w_l = (const uint32_t*)lv(G_WLAG, lane, 0); A.w_r = (const uint32_t*)lv(G_WLAG, lane, 1); A.w_o = (const uint32_t*)lv(G_WLAG, lane, 2);
        A.q_m = (const uint32_t*)q_lagrange[0]; A.q_l = (const uint32_t*)q_lagrange[1]; A.q_r = (const uint32_t*)q_lagrange[2];
        A.q_o = (const uint32_t*)q_lagrange[3]; A.q_c = (const uint32_t*)q_lagrange[4];
        A.q_on = has_seq ? (const uint32_t*)qs_lagrange : nullptr;
        if (has_bool) { A.q_bl = (const uint32_t*)qb_lagrange[0]; A.q_br = (const uint32_t*)qb_lagrange[1]; A.q_bo = (const uint32_t*)qb_lagrange[2]; }
        if (has_mimc) { A.q_sel = (const uint32_t*)qm_lagrange[0]; A.q_coef = (const uint32_t*)qm_lagrange[1]; }
        A.s1 = sigma_mapping[0]; A.s2 = sigma_mapping[1]; A.s3 = sigma_mapping[2];
        A.counts = check_counts + lane;
        A.first = check_first + lane;
        A.n = (uint32_t)n;
        return A;
    }
    // the two kernels over the first `count` lanes of the current set and the copy of their records, all on `st`
    int check_enqueue(int count)
    {
        RC(ensure_check());
        std::vector<poly::WitnessCheckArgs> ca((size_t)count);
        for (int l = 0; l < count; l++) ca[l] = check_args(l);
        RC(poly::check_witness_lanes(lane_tab, ca.data(), count, st));
        HIPCHK(d2h_async(h_check, check_counts, check_bytes, st));
        return BBGPU_OK;
    }
    // waits for the records and turns them into `reports`; with `verdict`, BBGPU_ERR_WITNESS when a lane fails
    int check_finish(int count, bool verdict)
    {
        report_count = 0;
        HIPCHK(hipStreamSynchronize(st));
        const poly::WitnessCheckCounts* hc = static_cast<const poly::WitnessCheckCounts*>(h_check);
        const poly::WitnessCheckFirst* hf = reinterpret_cast<const poly::WitnessCheckFirst*>(hc + BBGPU_PLONK_MAX_BATCH);
        for (int l = 0; l < count; l++) {
            bbgpu_plonk_witness_report R = host::plonk_report_clear();
            R.gate_failures = hc[l].gate_failures;
            R.copy_failures = hc[l].copy_failures;
            R.kinds = hc[l].kinds;
            if (hf[l].gate != ~0ull) {
                R.first_gate = (uint32_t)(hf[l].gate >> 32);
                R.first_gate_kinds = (uint32_t)hf[l].gate;
            }
            if (hf[l].copy != ~0ull) {
                const uint32_t key = (uint32_t)(hf[l].copy >> 32);
                R.first_copy = (key >> 2) | ((key & 3u) << 30);
                R.first_copy_target = (uint32_t)hf[l].copy;
            }
            reports[l] = R;
        }
        report_count = count;
        if (!verdict) return BBGPU_OK;
        for (int l = 0; l < count; l++) {
            const bbgpu_plonk_witness_report& R = reports[l];
            if (!R.gate_failures && !R.copy_failures) continue;
            if (R.gate_failures)
                set_error("witness of lane %d does not satisfy the circuit: gate identity (kinds 0x%x) fails in row %u (%llu failing rows, %llu failing copy constraints)",
                          l, R.first_gate_kinds, R.first_gate, (unsigned long long)R.gate_failures, (unsigned long long)R.copy_failures);
            else
                set_error("witness of lane %d does not satisfy the circuit: copy constraint of row %u, wire %u fails (mapping entry 0x%08x; %llu failing positions)", l,
                          R.first_copy & ((1u << 29) - 1u), R.first_copy >> 30, R.first_copy_target, (unsigned long long)R.copy_failures);
            return BBGPU_ERR_WITNESS;
        }
        return BBGPU_OK;
    }
    // the check alone: over the witness the handle holds ...
    int check_witness(bbgpu_plonk_witness_report* out)
    {
        use(own);
        RC(check_enqueue(1));
        RC(check_finish(1, false));
        *out = reports[0];
        return BBGPU_OK;
    }
    // ... and over `count` witnesses, loaded into the lanes a batch proof of the same count would use
    int check_witness_batch(int count, const bbgpu_plonk_witness* W, bbgpu_plonk_witness_report* out)
    {
        RC(ensure_lanes(count));
        use(batch);
        RC(load_lanes(count, W));
        RC(check_enqueue(count));
        RC(check_finish(count, false));
        memcpy(out, reports, sizeof(bbgpu_plonk_witness_report) * (size_t)count);
        return BBGPU_OK;
    }

    // ---- circuit-only state (first proof) -----------------------------------------------------------------------------
    int prepare_circuit()
    {
        if (circuit_ready) return BBGPU_OK;
        const double t0 = now_ms();
        const Fr root = host::fr_root_of_unity(log2n);
        // `batch` transforms of consecutive polynomials of `size` coefficients (the contiguous groups of init())
        auto ntts = [&](uint64_t* d, size_t size, int batch, int kind) { return bbgpu_ntt_device_batch(d, size, size, batch, kind, nullptr, st); };
        RC(poly::powers(roots, n, root, host::fr_one(), st));
        for (int k = 0; k < 3; k++) RC(poly::sigma_from_mapping(sigma_lagrange[k], sigma_mapping[k], roots, n, st)); // prover.cpp:663-665
        RC(copy(sigma_coeff, sigma_lagrange[0], 3 * n)); // prover.cpp:245-247 without the beta
        RC(ntts(sigma_coeff, n, 3, BBGPU_IFFT));
        // arithmetic_widget.cpp:68-84 without the alpha scaling (applied in quotient_mid)
        RC(copy(q_coeff[0], q_lagrange[0], 5 * n));
        RC(ntts(q_coeff[0], n, 5, BBGPU_IFFT));
        for (int k = 0; k < 5; k++) RC(poly::copy_pad(q_fft2n[k], q_coeff[k], n, 2 * n, st));
        RC(ntts(q_fft2n[0], 2 * n, 5, BBGPU_COSET_FFT));
        if (has_bool) { // bool_widget.cpp:64-74 without the alpha scalings (applied in quotient_bool)
            RC(copy(qb_coeff[0], qb_lagrange[0], 3 * n));
            RC(ntts(qb_coeff[0], n, 3, BBGPU_IFFT));
            for (int k = 0; k < 3; k++) RC(poly::copy_pad(qb_fft2n[k], qb_coeff[k], n, 2 * n, st));
            RC(ntts(qb_fft2n[0], 2 * n, 3, BBGPU_COSET_FFT));
        }
        if (has_seq) { // sequential_widget.cpp:49-54 without the alpha scaling (applied in quotient_seq)
            RC(copy(qs_coeff, qs_lagrange, n));
            RC(ntts(qs_coeff, n, 1, BBGPU_IFFT));
            RC(poly::copy_pad(qs_fft2n, qs_coeff, n, 2 * n, st));
            RC(ntts(qs_fft2n, 2 * n, 1, BBGPU_COSET_FFT));
        }
        if (has_mimc) { // mimc_widget.cpp:60-67 without the alpha scaling (applied in quotient_mimc)
            RC(copy(qm_coeff[0], qm_lagrange[0], 2 * n));
            RC(ntts(qm_coeff[0], n, 2, BBGPU_IFFT));
            for (int k = 0; k < 2; k++) RC(poly::copy_pad(qm_fft4n[k], qm_coeff[k], n, 4 * n, st));
            RC(ntts(qm_fft4n[0], 4 * n, 2, BBGPU_COSET_FFT));
        }
        RC(poly::lagrange_l1_fft(l_1, own.group[G_QM], log2n, log2n + 1, scratch, st)); // prover.cpp:350-351 (the own lane's quotient_mid as workspace)
        HIPCHK(hipStreamSynchronize(st));
        circuit_ready = true;
        timing[3] = now_ms() - t0;
        return BBGPU_OK;
    }

    // polynomial_arithmetic.cpp:594-626, l_1 only
    Fr lagrange_l1_at(const Fr& zc) const
    {
        Fr zp = zc;
        for (int i = 0; i < log2n; i++) zp = host::fr_sqr(zp);
        const Fr numerator = host::fr_mul(host::fr_sub(zp, host::fr_one()), host::fr_inv(host::fr_from_u64((uint64_t)n)));
        return host::fr_mul(numerator, host::fr_inv(host::fr_sub(zc, host::fr_one())));
    }
    // the evaluations of one proof, in the order of the jobs above (:478-515)
    void take_evaluations(Proof& proof, const Fr& beta_inv, const Fr ev[9], Fr* t_eval) const
    {
        if (has_mimc || has_seq) proof.w_o_shifted_eval = ev[7];
        if (has_mimc) proof.q_mimc_coefficient_eval = ev[8];
        proof.w_l_eval = ev[0];
        proof.w_r_eval = ev[1];
        proof.w_o_eval = ev[2];
        proof.sigma_1_eval = host::fr_mul(ev[3], beta_inv); // :514-515
        proof.sigma_2_eval = host::fr_mul(ev[4], beta_inv);
        proof.z_1_shifted_eval = ev[5];
        *t_eval = ev[6];
    }
    // r as a linear combination of resident vectors: Z and beta S_3 (`z_poly`, `sigma3_poly`: the proof's own) and the circuit's selectors; returns the
    // number of terms, pointers in pl, coefficients in cl
    int linearisation_terms(const Proof& proof, const Challenges& challenges, const Fr& beta_inv, const uint64_t* z_poly, const uint64_t* sigma3_poly,
                            const uint64_t* pl[12], Fr cl[12]) const
    {
        const Fr& zc = challenges.z;
        // linearizer.hpp:29-83
        const Fr k1 = host::fr_from_limbs(FrHostP::GEN5), k2 = host::fr_from_limbs(FrHostP::GEN7);
        const Fr &alpha = challenges.alpha, &beta = challenges.beta, &gamma = challenges.gamma;
        const Fr alpha3 = host::fr_mul(host::fr_sqr(alpha), alpha);
        const Fr zb = host::fr_mul(zc, beta);
        Fr T0 = host::fr_add(host::fr_add(zb, proof.w_l_eval), gamma);
        Fr T1 = host::fr_add(host::fr_add(host::fr_mul(zb, k1), proof.w_r_eval), gamma);
        Fr T2 = host::fr_add(host::fr_add(host::fr_mul(zb, k2), proof.w_o_eval), gamma);
        Fr lt_z1 = host::fr_mul(host::fr_mul(host::fr_mul(T2, T1), T0), alpha);
        T0 = host::fr_add(host::fr_add(host::fr_mul(proof.sigma_1_eval, beta), proof.w_l_eval), gamma);
        T1 = host::fr_add(host::fr_add(host::fr_mul(proof.sigma_2_eval, beta), proof.w_r_eval), gamma);
        Fr lt_sigma3 = host::fr_mul(host::fr_neg(host::fr_mul(host::fr_mul(host::fr_mul(T1, T0), proof.z_1_shifted_eval), alpha)), beta);
        lt_z1 = host::fr_add(lt_z1, host::fr_mul(lagrange_l1_at(zc), alpha3));

        // :520-528 and arithmetic_widget.cpp:106-126 in one pass: r = z_1 Z + (sigma_3 / beta)(beta S_3) + alpha^4 (...selectors...)
        const Fr alpha4 = host::fr_sqr(host::fr_sqr(alpha));
        const Fr w_lr = host::fr_mul(proof.w_l_eval, proof.w_r_eval);
        const uint64_t* ps[10] = { z_poly, sigma3_poly, q_coeff[0], q_coeff[1], q_coeff[2], q_coeff[3], q_coeff[4], qb_coeff[0], qb_coeff[1], qb_coeff[2] };
        // bool_widget.cpp:106-124: (w^2 - w) alpha^5, alpha^6, alpha^7 on q_bl, q_br, q_bo
        const Fr alpha5 = host::fr_mul(alpha4, alpha), alpha6 = host::fr_mul(alpha5, alpha), alpha7 = host::fr_mul(alpha6, alpha);
        auto boolmul = [](const Fr& e, const Fr& a) { return host::fr_mul(host::fr_sub(host::fr_sqr(e), e), a); };
        const Fr cs[10] = { lt_z1, host::fr_mul(lt_sigma3, beta_inv), host::fr_mul(w_lr, alpha4), host::fr_mul(proof.w_l_eval, alpha4),
                            host::fr_mul(proof.w_r_eval, alpha4), host::fr_mul(proof.w_o_eval, alpha4), alpha4,
                            boolmul(proof.w_l_eval, alpha5), boolmul(proof.w_r_eval, alpha6), boolmul(proof.w_o_eval, alpha7) };
        int terms = 7;
        for (int j = 0; j < 7; j++) { pl[j] = ps[j]; cl[j] = cs[j]; }
        if (has_seq) { // sequential_widget.cpp:64-74: w_o(z omega) * alpha^4 on q_o_next
            pl[terms] = qs_coeff;
            cl[terms++] = host::fr_mul(proof.w_o_shifted_eval, alpha4);
        }
        if (has_bool)
            for (int j = 7; j < 10; j++) { pl[terms] = ps[j]; cl[terms++] = cs[j]; }
        if (has_mimc) { // mimc_widget.cpp:97-113 with alpha_base = alpha^5, alpha_step = alpha
            const Fr t0 = host::fr_add(host::fr_add(proof.w_o_eval, proof.w_l_eval), proof.q_mimc_coefficient_eval);
            const Fr a = host::fr_sub(host::fr_mul(host::fr_sqr(t0), t0), proof.w_r_eval);
            const Fr b = host::fr_mul(host::fr_sub(host::fr_mul(host::fr_sqr(proof.w_r_eval), t0), proof.w_o_shifted_eval), alpha);
            pl[terms] = qm_coeff[0];
            cl[terms++] = host::fr_mul(host::fr_add(b, a), alpha5);
        }
        return terms;
    }
    static Fr nu_challenge(const Proof& proof, const Fr& t_eval)
    {
        std::vector<uint64_t> b = transcript_of(proof, 2); // compute_linearisation_challenge, challenge.hpp:114-125
        put_fr(b, proof.w_l_eval); put_fr(b, proof.w_r_eval); put_fr(b, proof.w_o_eval);
        put_fr(b, proof.sigma_1_eval); put_fr(b, proof.sigma_2_eval); put_fr(b, proof.z_1_shifted_eval);
        put_fr(b, proof.linear_eval); put_fr(b, t_eval);
        return challenge(b);
    }
    // waffle::preprocess(prover) (preprocess.hpp:16-55) + ProverArithmeticWidget::compute_preprocessed_commitments
    // (arithmetic_widget.cpp:128-157): the verification key -- commitments to sigma_1..3 and to q_m, q_l, q_r, q_o, q_c, then the widgets' selectors
    int preprocess(uint64_t (*out)[8])
    {
        RC(prepare_circuit());
        PendingMany P;
        for (int k = 0; k < 3; k++) P.scalars.push_back(sigma_coeff + (size_t)k * n * 4);
        for (int k = 0; k < 5; k++) P.scalars.push_back(q_coeff[k]);
        if (has_seq) P.scalars.push_back(qs_coeff); // sequential_widget.cpp:79-106, second widget of the ExtendedComposer's chain
        if (has_bool)                               // bool_widget.cpp:118-152
            for (int k = 0; k < 3; k++) P.scalars.push_back(qb_coeff[k]);
        if (has_mimc) { // mimc_widget.cpp:125-160: q_mimc_coefficient first, then q_mimc_selector
            P.scalars.push_back(qm_coeff[1]);
            P.scalars.push_back(qm_coeff[0]);
        }
        RC(commit_many_begin(P));
        return commit_many_end(P, out, &timing[1]);
    }

    // ==== the rounds, advanced in lockstep over the lanes of the current set ===========================================================================
    // The circuit-only state above is shared by all lanes.  Each host synchronisation point of waffle::Prover::construct_proof is reached once per run:
    // the device work of all lanes is enqueued, then the host finishes every lane's commitments, hashes every lane's transcript and enqueues the next round.
    size_t lane_bytes() const { return (size_t)batch.count * (48 * n * 32 + 16 * 32); }
    void release_lanes()
    {
        for (uint64_t*& g : batch.group) {
            if (g) (void)dev_free(g);
            g = nullptr;
        }
        release_vars(batch);
        if (batch.slots) (void)dev_free(batch.slots);
        batch.slots = nullptr;
        g_lane_bytes -= lane_bytes();
        batch.count = 0;
    }
    // the set the calls below address; the table's regions are free again (every entry leaves `st` idle)
    void use(LaneSet& s)
    {
        cur = &s;
        lane_tab.reset();
    }
    // vector k of group g of lane l
    uint64_t* lv(int g, int l, int k = 0) const { return cur->group[g] + ((size_t)l * lane_group_vectors[g] + k) * n * 4; }
    uint64_t* lslot(int l, int k) const { return cur->slots + ((size_t)l * 16 + k) * 4; }
    int ensure_lanes(int count)
    {
        if (count <= batch.count) return BBGPU_OK;
        HIPCHK(hipStreamSynchronize(st));
        release_lanes(); // nothing of a lane outlives its batch: a larger count starts over
        batch.count = count;
        g_lane_bytes += lane_bytes();
        int rc = BBGPU_OK;
        for (int g = 0; g < G_COUNT && !rc; g++)
            if (dev_malloc((void**)&batch.group[g], (size_t)count * lane_group_vectors[g] * n * 32) != hipSuccess) rc = BBGPU_ERR_HIP;
        if (!rc && dev_malloc((void**)&batch.slots, (size_t)count * 16 * 32) != hipSuccess) rc = BBGPU_ERR_HIP;
        if (rc) release_lanes(); // a refused allocation gives back the groups it had got
        return rc;
    }

    // `total` commitments over n scalars each, as batch tickets of up to MSM_MAX_JOBS jobs on queues of their own behind `scalars_ready`; over an SRS
    // without window tables, single tickets.  As many tickets as there are free slots go out at once; the rest follows when those are collected.
    // Tickets that were issued and never waited on would stay `pending` for the life of the process and turn every later host-pointer MSM into
    // BBGPU_ERR_STATE: whatever happens between begin and end (a failing transform, a failing later ticket), the destructor collects what is still
    // outstanding.  Work that does not depend on a round's challenge is enqueued on `st` between begin and end: a 2^16-point batch is a ~0.4 ms chain of
    // mostly latency-bound launches on the MSMs' own queues, beside which transforms run almost for free.
    struct PendingMany {
        struct Tk { int ticket, first, jobs; bool batched; };
        std::vector<Tk> held;
        std::vector<const uint64_t*> scalars;
        int next = 0, streams = 0;
        bool batched = true;
        double t0 = 0.0;
        PendingMany() = default;
        PendingMany(const PendingMany&) = delete;
        PendingMany& operator=(const PendingMany&) = delete;
        ~PendingMany() { drain(); }
        void drain()
        {
            uint64_t sink[4 * 12];
            for (const Tk& t : held) (void)(t.batched ? bbgpu_msm_g1_batch_wait(t.ticket, sink) : bbgpu_msm_g1_wait(t.ticket, sink));
            held.clear();
        }
    };
    // issues tickets until everything is out or no slot is free
    int commit_many_issue(PendingMany& P)
    {
        const int total = (int)P.scalars.size();
        while (P.next < total) {
            hipStream_t q = st_ticket[P.streams % 8];
            int t, jobs;
            if (P.batched) {
                jobs = std::min(total - P.next, (int)MSM_MAX_JOBS);
                HIPCHK(hipStreamWaitEvent(q, scalars_ready, 0));
                t = bbgpu_msm_g1_device_batch_async(srs, 0, P.scalars.data() + P.next, jobs, n, q);
                if (t == BBGPU_ERR_ARG && P.held.empty() && P.next == 0) { // no window tables on this SRS: side-by-side single MSMs
                    P.batched = false;
                    continue;
                }
            } else {
                jobs = 1;
                const int W = bbgpu_srs_num_windows(srs, n);
                if (W < 0) return W;
                HIPCHK(hipStreamWaitEvent(q, scalars_ready, 0));
                t = bbgpu_msm_g1_device_async(srs, 0, P.scalars[P.next], n, 0, W, q);
            }
            if (t == BBGPU_ERR_STATE && !P.held.empty()) return BBGPU_OK; // every free slot is taken: collect first
            if (t < 0) return t;
            P.held.push_back({ t, P.next, jobs, P.batched });
            P.next += jobs;
            P.streams++;
        }
        return BBGPU_OK;
    }
    int commit_many_begin(PendingMany& P)
    {
        P.t0 = now_ms();
        HIPCHK(hipEventRecord(scalars_ready, st)); // the scalars are produced on `st`
        return commit_many_issue(P);
    }
    int commit_many_end(PendingMany& P, uint64_t (*out)[8], double* msm_ms)
    {
        uint64_t res[4 * 12];
        for (;;) {
            while (!P.held.empty()) {
                const PendingMany::Tk t = P.held.front();
                P.held.erase(P.held.begin()); // a wait consumes the ticket whatever it returns
                RC(t.batched ? bbgpu_msm_g1_batch_wait(t.ticket, res) : bbgpu_msm_g1_wait(t.ticket, res));
                for (int i = 0; i < t.jobs; i++) memcpy(out[t.first + i], res + 12 * i, 64); // normalised: x, y canonical
            }
            if (P.next >= (int)P.scalars.size()) break;
            RC(commit_many_issue(P));
        }
        *msm_ms += now_ms() - P.t0;
        return BBGPU_OK;
    }
    int read_lane_slots(int count)
    {
        HIPCHK(d2h_async(h_lane_slots, cur->slots, (size_t)count * 16 * 32, st));
        HIPCHK(hipStreamSynchronize(st));
        return BBGPU_OK;
    }
    Fr host_slot(int l, int k) const
    {
        Fr v;
        memcpy(v.d, (const uint8_t*)h_lane_slots + ((size_t)l * 16 + k) * 32, 32);
        return v;
    }

    // Round 0: lane l's Lagrange-form wires (G_WLAG of the current set) from witness l in whatever form and place it comes.  Expanded host wires are three uploads
    // per lane, as ever; expanded device wires three device copies; variables one upload per lane (none from device memory: the expansion reads the
    // caller's buffer) and ONE expansion launch for all such lanes.  The caller's buffers are last read by work enqueued here, and every entry that
    // calls this synchronises `st` before it returns.
    int load_lanes(int L, const bbgpu_plonk_witness* W)
    {
        bool host_variables = false;
        for (int l = 0; l < L; l++) {
            host_variables |= W[l].form == BBGPU_PLONK_WITNESS_VARIABLES && W[l].where == BBGPU_PLONK_WITNESS_HOST;
            if (W[l].where == BBGPU_PLONK_WITNESS_DEVICE && (l == 0 || W[l - 1].where != BBGPU_PLONK_WITNESS_DEVICE || W[l - 1].hip_stream != W[l].hip_stream))
                RC(wait_for_caller(W[l].hip_stream));
        }
        if (host_variables && !cur->vars) { // sized for every lane of the set: the batch set's goes with its lanes when they grow (ensure_lanes)
            const size_t bytes = (size_t)cur->count * num_variables * 32;
            HIPCHK(dev_malloc((void**)&cur->vars, bytes));
            cur->vars_bytes = bytes;
            g_lane_bytes += bytes;
        }
        std::vector<poly::ExpandWiresArgs> ex;
        for (int l = 0; l < L; l++) {
            const uint64_t* hw[3] = { W[l].w_l, W[l].w_r, W[l].w_o };
            if (W[l].form == BBGPU_PLONK_WITNESS_WIRES) {
                for (int k = 0; k < 3; k++)
                    RC(W[l].where == BBGPU_PLONK_WITNESS_HOST ? host_to_device(lv(G_WLAG, l, k), hw[k], n * 32, st) : copy(lv(G_WLAG, l, k), hw[k], n));
                continue;
            }
            const uint64_t* src = W[l].variables;
            if (W[l].where == BBGPU_PLONK_WITNESS_HOST) {
                uint64_t* stage = cur->vars + (size_t)l * num_variables * 4;
                RC(host_to_device(stage, W[l].variables, num_variables * 32, st));
                src = stage;
            }
            uint64_t* const dst[3] = { lv(G_WLAG, l, 0), lv(G_WLAG, l, 1), lv(G_WLAG, l, 2) };
            ex.push_back(expand_args(src, dst));
        }
        if (!ex.empty()) RC(poly::expand_wires_lanes(lane_tab, ex.data(), (int)ex.size(), st));
        return BBGPU_OK;
    }

    // waffle::Prover::construct_proof (prover.cpp:661-670) over the first L lanes of the current set; the finished proofs and challenges are left in
    // `lanes`.  W: the L witnesses to load first, or null when the wires are in the lanes already.  tm: total, msm, the rest, first-use preparation.
    int prove(int L, const bbgpu_plonk_witness* W, double tm[4])
    {
        tm[0] = tm[1] = tm[2] = 0;
        RC(prepare_circuit());
        const double t0 = now_ms();
        lanes.assign((size_t)L, Lane{});
        const size_t n4 = 4 * n, n2 = 2 * n;
        std::vector<Fr> fa((size_t)3 * L), fb((size_t)3 * L), fc((size_t)L);
        std::vector<uint64_t> pts((size_t)3 * L * 8);
        uint64_t(*out)[8] = reinterpret_cast<uint64_t(*)[8]>(pts.data());

        // ---- round 1: wires (prover.cpp:124-133, :65-86)
        if (W) RC(load_lanes(L, W));
        if (witness_check) RC(check_enqueue(L)); // opt-in: beside the inverse transforms, the verdict before the first commitment is issued
        RC(copy(lv(G_W, 0), lv(G_WLAG, 0), (size_t)3 * L * n));
        RC(bbgpu_ntt_device_batch(lv(G_W, 0), n, n, 3 * L, BBGPU_IFFT, nullptr, st));
        if (witness_check) RC(check_finish(L, true));
        {
            PendingMany P;
            for (int l = 0; l < L; l++)
                for (int k = 0; k < 3; k++) P.scalars.push_back(lv(G_W, l, k));
            RC(commit_many_begin(P));
            // beside the commitments: the wires on the 4n coset (prover.cpp:418-425) need no challenge
            std::vector<poly::CopyPadArgs> cp((size_t)3 * L);
            for (int l = 0; l < L; l++)
                for (int k = 0; k < 3; k++) {
                    poly::CopyPadArgs& C = cp[(size_t)l * 3 + k];
                    C = poly::CopyPadArgs{};
                    C.dst = (uint32_t*)(lv(G_WFFT, l) + (size_t)k * n4 * 4);
                    C.src = (const uint32_t*)lv(G_W, l, k);
                    C.n_src = (uint32_t)n;
                    C.n_dst = (uint32_t)n4;
                }
            RC(poly::copy_pad_lanes(lane_tab, cp.data(), 3 * L, nullptr, st));
            RC(bbgpu_ntt_device_batch(lv(G_WFFT, 0), n4, n4, 3 * L, BBGPU_COSET_FFT, nullptr, st));
            RC(commit_many_end(P, out, &tm[1]));
        }
        for (int l = 0; l < L; l++) {
            Lane& X = lanes[l];
            memcpy(X.proof.W_L, out[3 * l], 64);
            memcpy(X.proof.W_R, out[3 * l + 1], 64);
            memcpy(X.proof.W_O, out[3 * l + 2], 64);
            std::vector<uint64_t> b = transcript_of(X.proof, 0);
            X.ch.gamma = challenge(b); // compute_gamma, challenge.hpp:64-73
            put_fr(b, X.ch.gamma);
            X.ch.beta = challenge(b);  // compute_beta, :75-85
            fa[l] = X.ch.beta;
            fb[l] = X.ch.gamma;
        }

        // ---- round 2: the grand product (prover.cpp:135-222, :88-105): Z(w^m) = prod_{i<m} num_i / den_i.  The six serial accumulator chains (:194-202)
        // and the batch inversion (:215) become one exclusive prefix-product scan of the numerators (-> G_TMP 2), one inclusive suffix-product scan of the
        // denominators (-> G_R, free at this point; total -> slot 0) and a single inversion: 1 / prod_{i<m} den_i = (prod_{i>=m} den_i) / prod_i den_i.
        {
            std::vector<poly::ZTermsArgs> za((size_t)L);
            std::vector<poly::ScanJob> sj((size_t)2 * L);
            for (int l = 0; l < L; l++) {
                poly::ZTermsArgs& A = za[l];
                A = poly::ZTermsArgs{};
                A.w_l = (const uint32_t*)lv(G_WLAG, l, 0); A.w_r = (const uint32_t*)lv(G_WLAG, l, 1); A.w_o = (const uint32_t*)lv(G_WLAG, l, 2);
                A.s1 = (const uint32_t*)sigma_lagrange[0]; A.s2 = (const uint32_t*)sigma_lagrange[1]; A.s3 = (const uint32_t*)sigma_lagrange[2];
                A.num = (uint32_t*)lv(G_TMP, l, 0); A.den = (uint32_t*)lv(G_TMP, l, 1);
                A.n = (uint32_t)n;
                poly::ScanJob &pn = sj[(size_t)2 * l], &sd = sj[(size_t)2 * l + 1];
                pn = poly::ScanJob{};
                sd = poly::ScanJob{};
                pn.in = lv(G_TMP, l, 0); pn.out = lv(G_TMP, l, 2); pn.n = n; pn.reverse = false; pn.inclusive = false;
                sd.in = lv(G_TMP, l, 1); sd.out = lv(G_R, l); sd.n = n; sd.reverse = true; sd.inclusive = true; sd.d_total = lslot(l, 0);
            }
            RC(poly::z_terms_lanes(lane_tab, za.data(), L, host::fr_root_of_unity(log2n), fa.data(), fb.data(), st));
            RC(poly::scan_lanes(0, sj.data(), 2 * L, lane_tab, scratch, st));
            RC(read_lane_slots(L));
            std::vector<poly::Mul2cArgs> ma((size_t)L);
            for (int l = 0; l < L; l++) {
                ma[l] = poly::Mul2cArgs{};
                ma[l].out = (uint32_t*)lv(G_Z, l);
                ma[l].a = (const uint32_t*)lv(G_TMP, l, 2);
                ma[l].b = (const uint32_t*)lv(G_R, l);
                ma[l].n = (uint32_t)n;
                fc[l] = host::fr_inv(host_slot(l, 0));
            }
            RC(poly::mul2c_lanes(lane_tab, ma.data(), L, fc.data(), st));
            RC(bbgpu_ntt_device_batch(lv(G_Z, 0), n, n, L, BBGPU_IFFT, nullptr, st));
        }
        {
            PendingMany P;
            for (int l = 0; l < L; l++) P.scalars.push_back(lv(G_Z, l));
            RC(commit_many_begin(P));
            // beside the commitment: the permutation polynomials need beta and gamma only (prover.cpp:245-247, :253-276).  beta sigma_i comes from the
            // circuit's unscaled coefficient form, scaled per lane; the 4n transform is the plain kind, shared by all lanes
            std::vector<poly::CopyPadArgs> cp((size_t)3 * L);
            std::vector<poly::SigmaPrepArgs> sp((size_t)3 * L);
            for (int l = 0; l < L; l++)
                for (int k = 0; k < 3; k++) {
                    const size_t i = (size_t)l * 3 + k;
                    cp[i] = poly::CopyPadArgs{};
                    cp[i].dst = (uint32_t*)lv(G_SIGMA, l, k);
                    cp[i].src = (const uint32_t*)(sigma_coeff + (size_t)k * n * 4);
                    cp[i].n_src = cp[i].n_dst = (uint32_t)n;
                    sp[i] = poly::SigmaPrepArgs{};
                    sp[i].dst = (uint32_t*)(lv(G_SFFT, l) + (size_t)k * n4 * 4);
                    sp[i].sigma = (const uint32_t*)lv(G_SIGMA, l, k);
                    sp[i].w = (const uint32_t*)lv(G_W, l, k);
                    sp[i].n = (uint32_t)n;
                    sp[i].n_dst = (uint32_t)n4;
                    fa[i] = lanes[l].ch.beta;
                    fb[i] = lanes[l].ch.gamma;
                }
            RC(poly::copy_pad_lanes(lane_tab, cp.data(), 3 * L, fa.data(), st));
            RC(poly::sigma_prepare_lanes(lane_tab, sp.data(), 3 * L, fb.data(), st));
            RC(bbgpu_ntt_device_batch(lv(G_SFFT, 0), n4, n4, 3 * L, BBGPU_COSET_FFT, nullptr, st));
            RC(commit_many_end(P, out, &tm[1]));
        }
        for (int l = 0; l < L; l++) {
            memcpy(lanes[l].proof.Z_1, out[l], 64);
            lanes[l].ch.alpha = challenge(transcript_of(lanes[l].proof, 1)); // compute_alpha, challenge.hpp:87-98
        }

        // ---- round 3: the quotient.  prover.cpp:224-300 + :302-341 fused into one pass over the 4n coset, :350-402 + arithmetic_widget.cpp:66-104 into one
        // over the 2n coset, then :405-465 and the commitments of :107-122.  G_WFFT and G_SFFT were enqueued beside the wire / Z commitments.
        {
            std::vector<poly::CopyPadArgs> cp((size_t)L);
            std::vector<poly::QuotLargeArgs> la((size_t)L);
            std::vector<poly::QuotMidArgs> mi((size_t)L);
            std::vector<Fr> alpha((size_t)L), abase((size_t)L), a5((size_t)L), a6((size_t)L), a7((size_t)L), beta((size_t)L), gamma((size_t)L);
            for (int l = 0; l < L; l++) {
                const uint64_t* wf = lv(G_WFFT, l);
                const uint64_t* sf = lv(G_SFFT, l);
                alpha[l] = lanes[l].ch.alpha;
                beta[l] = lanes[l].ch.beta;
                gamma[l] = lanes[l].ch.gamma;
                abase[l] = host::fr_sqr(host::fr_sqr(alpha[l])); // :446-451
                a5[l] = host::fr_mul(abase[l], alpha[l]);
                a6[l] = host::fr_mul(a5[l], alpha[l]);
                a7[l] = host::fr_mul(a6[l], alpha[l]);
                cp[l] = poly::CopyPadArgs{}; // alpha Z, padded (:440, :278: the scaling moved in front of the shared plain transform)
                cp[l].dst = (uint32_t*)lv(G_ZFFT, l);
                cp[l].src = (const uint32_t*)lv(G_Z, l);
                cp[l].n_src = (uint32_t)n;
                cp[l].n_dst = (uint32_t)n4;
                poly::QuotLargeArgs& A = la[l];
                A = poly::QuotLargeArgs{};
                A.wl_f = (const uint32_t*)wf; A.wr_f = (const uint32_t*)(wf + n4 * 4); A.wo_f = (const uint32_t*)(wf + 2 * n4 * 4);
                A.s1_f = (const uint32_t*)sf; A.s2_f = (const uint32_t*)(sf + n4 * 4); A.s3_f = (const uint32_t*)(sf + 2 * n4 * 4);
                A.z_f = (const uint32_t*)lv(G_ZFFT, l);
                A.q = (uint32_t*)lv(G_QL, l);
                A.n4 = (uint32_t)n4;
                poly::QuotMidArgs& M = mi[l];
                M = poly::QuotMidArgs{};
                M.z_f = A.z_f;
                M.wl_f = A.wl_f; M.wr_f = A.wr_f; M.wo_f = A.wo_f;
                M.l1 = (const uint32_t*)l_1;
                M.qm_f = (const uint32_t*)q_fft2n[0]; M.ql_f = (const uint32_t*)q_fft2n[1]; M.qr_f = (const uint32_t*)q_fft2n[2];
                M.qo_f = (const uint32_t*)q_fft2n[3]; M.qc_f = (const uint32_t*)q_fft2n[4];
                M.q = (uint32_t*)lv(G_QM, l);
                M.n2 = (uint32_t)n2;
            }
            RC(poly::copy_pad_lanes(lane_tab, cp.data(), L, alpha.data(), st));
            RC(bbgpu_ntt_device_batch(lv(G_ZFFT, 0), n4, n4, L, BBGPU_COSET_FFT, nullptr, st));
            RC(poly::quotient_large_lanes(lane_tab, la.data(), L, host::fr_root_of_unity(log2n + 2), beta.data(), gamma.data(), st));
            RC(poly::quotient_mid_lanes(lane_tab, mi.data(), L, alpha.data(), abase.data(), st));
            if (has_seq) { // sequential_widget.cpp:47-62
                std::vector<poly::QuotSeqArgs> sq((size_t)L);
                for (int l = 0; l < L; l++) {
                    sq[l] = poly::QuotSeqArgs{};
                    sq[l].wo_f = mi[l].wo_f;
                    sq[l].qon_f = (const uint32_t*)qs_fft2n;
                    sq[l].q = mi[l].q;
                    sq[l].n2 = (uint32_t)n2;
                }
                RC(poly::quotient_seq_lanes(lane_tab, sq.data(), L, abase.data(), st));
            }
            if (has_bool) {
                std::vector<poly::QuotBoolArgs> bq((size_t)L);
                for (int l = 0; l < L; l++) {
                    bq[l] = poly::QuotBoolArgs{};
                    bq[l].wl_f = mi[l].wl_f; bq[l].wr_f = mi[l].wr_f; bq[l].wo_f = mi[l].wo_f;
                    bq[l].qbl_f = (const uint32_t*)qb_fft2n[0]; bq[l].qbr_f = (const uint32_t*)qb_fft2n[1]; bq[l].qbo_f = (const uint32_t*)qb_fft2n[2];
                    bq[l].q = mi[l].q;
                    bq[l].n2 = (uint32_t)n2;
                }
                RC(poly::quotient_bool_lanes(lane_tab, bq.data(), L, a5.data(), a6.data(), a7.data(), st));
            }
            if (has_mimc) {
                std::vector<poly::QuotMimcArgs> mq((size_t)L);
                for (int l = 0; l < L; l++) {
                    mq[l] = poly::QuotMimcArgs{};
                    mq[l].wl_f = la[l].wl_f; mq[l].wr_f = la[l].wr_f; mq[l].wo_f = la[l].wo_f;
                    mq[l].qsel_f = (const uint32_t*)qm_fft4n[0]; mq[l].qcoef_f = (const uint32_t*)qm_fft4n[1];
                    mq[l].q = la[l].q;
                    mq[l].n4 = (uint32_t)n4;
                }
                RC(poly::quotient_mimc_lanes(lane_tab, mq.data(), L, a5.data(), alpha.data(), st));
            }
            RC(poly::divide_by_pseudo_vanishing_lanes(lv(G_QM, 0), n2, L, log2n, log2n + 1, st)); // :453
            RC(poly::divide_by_pseudo_vanishing_lanes(lv(G_QL, 0), n4, L, log2n, log2n + 2, st)); // :454
            RC(bbgpu_ntt_device_batch(lv(G_QM, 0), n2, n2, L, BBGPU_COSET_IFFT, nullptr, st));      // :457
            RC(bbgpu_ntt_device_batch(lv(G_QL, 0), n4, n4, L, BBGPU_COSET_IFFT, nullptr, st));      // :458
            RC(poly::add_inplace_lanes(lv(G_QL, 0), n4, lv(G_QM, 0), n2, n2, L, st));               // :461-463
        }
        {
            PendingMany P;
            for (int l = 0; l < L; l++)
                for (int k = 0; k < 3; k++) P.scalars.push_back(lv(G_QL, l) + (size_t)k * n * 4);
            RC(commit_many_begin(P));
            RC(commit_many_end(P, out, &tm[1]));
        }
        for (int l = 0; l < L; l++) {
            memcpy(lanes[l].proof.T_LO, out[3 * l], 64);
            memcpy(lanes[l].proof.T_MID, out[3 * l + 1], 64);
            memcpy(lanes[l].proof.T_HI, out[3 * l + 2], 64);
            lanes[l].ch.z = challenge(transcript_of(lanes[l].proof, 2)); // compute_evaluation_challenge, challenge.hpp:100-112
        }

        // ---- round 4: evaluations and the linearisation polynomial (prover.cpp:467-538): the evaluations of all lanes in one pair of launches and one
        // read-back (:478-480, :504-506, :512; with the MiMC or the sequential widget w_o at z omega, REQUIRES_W_O_SHIFTED, prover.cpp:499-502,
        // sequential_widget.cpp:16, and with the MiMC widget q_mimc_coefficient, mimc_widget.cpp:92-95), then r and its evaluation (:536)
        const int nev = has_mimc ? 9 : has_seq ? 8 : 7;
        const Fr omega = host::fr_root_of_unity(log2n);
        std::vector<Fr> zs((size_t)2 * L);
        {
            std::vector<poly::EvalJob> ej((size_t)nev * L);
            std::vector<int> zi((size_t)nev * L);
            for (int l = 0; l < L; l++) {
                zs[(size_t)2 * l] = lanes[l].ch.z;
                zs[(size_t)2 * l + 1] = host::fr_mul(lanes[l].ch.z, omega);
                const poly::EvalJob jl[9] = { { lv(G_W, l, 0), n, 0, lslot(l, 0) }, { lv(G_W, l, 1), n, 0, lslot(l, 1) }, { lv(G_W, l, 2), n, 0, lslot(l, 2) },
                                              { lv(G_SIGMA, l, 0), n, 0, lslot(l, 3) }, { lv(G_SIGMA, l, 1), n, 0, lslot(l, 4) }, { lv(G_Z, l), n, 1, lslot(l, 5) },
                                              { lv(G_QL, l), 3 * n, 0, lslot(l, 6) }, { lv(G_W, l, 2), n, 1, lslot(l, 7) }, { qm_coeff[1], n, 0, lslot(l, 8) } };
                for (int j = 0; j < nev; j++) {
                    ej[(size_t)l * nev + j] = jl[j];
                    zi[(size_t)l * nev + j] = 2 * l + jl[j].zsel;
                }
            }
            RC(poly::evaluate_lanes(ej.data(), zi.data(), nev * L, zs.data(), 2 * L, lane_tab, scratch, st));
            RC(read_lane_slots(L));
            std::vector<poly::LinCombArgs> lc((size_t)L);
            std::vector<Fr> cl((size_t)12 * L);
            std::vector<poly::EvalJob> rj((size_t)L);
            std::vector<int> rz((size_t)L);
            for (int l = 0; l < L; l++) {
                Fr ev[9];
                for (int j = 0; j < nev; j++) ev[j] = host_slot(l, j);
                lanes[l].beta_inv = host::fr_inv(lanes[l].ch.beta);
                take_evaluations(lanes[l].proof, lanes[l].beta_inv, ev, &lanes[l].t_eval);
                const uint64_t* pl[12];
                const int terms = linearisation_terms(lanes[l].proof, lanes[l].ch, lanes[l].beta_inv, lv(G_Z, l), lv(G_SIGMA, l, 2), pl, &cl[(size_t)12 * l]);
                lc[l] = poly::LinCombArgs{};
                for (int j = 0; j < terms; j++) lc[l].p[j] = (const uint32_t*)pl[j];
                lc[l].count = terms;
                lc[l].out = (uint32_t*)lv(G_R, l);
                lc[l].n = (uint32_t)n;
                rj[l] = poly::EvalJob{ lv(G_R, l), n, 0, lslot(l, 9) };
                rz[l] = 2 * l;
            }
            RC(poly::lincomb_lanes(lane_tab, lc.data(), L, cl.data(), st));
            RC(poly::evaluate_lanes(rj.data(), rz.data(), L, zs.data(), 2 * L, lane_tab, scratch, st)); // :536
            RC(read_lane_slots(L));
        }

        // ---- round 5: the opening polynomials (prover.cpp:540-659).  :567-595 is one linear combination of nine resident vectors; with the MiMC or the
        // sequential widget w_o joins the shifted opening at nu^8 (:627-635) and q_mimc_coefficient the main one at nu^9 (mimc_widget.cpp:115-123).
        // compute_kate_opening_coefficients (polynomial_arithmetic.cpp:562-591): W_i = sum_{j>i} F_j z^(j-i-1); the serial recurrence becomes a Horner
        // suffix scan, the remainder F(z) drops out.
        {
            std::vector<poly::LinCombArgs> oa((size_t)L), ob((size_t)L);
            std::vector<Fr> ca((size_t)12 * L), cb((size_t)12 * L);
            std::vector<poly::ScanJob> kj((size_t)2 * L);
            const int oterms = has_mimc ? 10 : 9;
            for (int l = 0; l < L; l++) {
                Lane& X = lanes[l];
                X.proof.linear_eval = host_slot(l, 9);
                X.ch.nu = nu_challenge(X.proof, X.t_eval);
                Fr nu[8];
                nu[0] = X.ch.nu;
                for (int i = 1; i < 8; i++) nu[i] = host::fr_mul(nu[i - 1], nu[0]);
                const Fr& beta_inv = X.beta_inv;
                const Fr z_pow_n = host::fr_pow(X.ch.z, (uint64_t)n), z_pow_2n = host::fr_pow(X.ch.z, (uint64_t)2 * n);
                const Fr nu9 = host::fr_mul(nu[7], nu[0]);
                const uint64_t* ql = lv(G_QL, l);
                const uint64_t* ps[10] = { ql, ql + n * 4, ql + 2 * n * 4, lv(G_R, l), lv(G_W, l, 0), lv(G_W, l, 1), lv(G_W, l, 2), lv(G_SIGMA, l, 0), lv(G_SIGMA, l, 1),
                                           qm_coeff[1] };
                const Fr cs[10] = { host::fr_one(), z_pow_n, z_pow_2n, nu[0], nu[1], nu[2], nu[3], host::fr_mul(nu[4], beta_inv), host::fr_mul(nu[5], beta_inv), nu9 };
                oa[l] = poly::LinCombArgs{};
                for (int j = 0; j < oterms; j++) {
                    oa[l].p[j] = (const uint32_t*)ps[j];
                    ca[(size_t)12 * l + j] = cs[j];
                }
                oa[l].count = oterms;
                oa[l].out = (uint32_t*)lv(G_TMP, l, 0);
                oa[l].n = (uint32_t)n;
                ob[l] = poly::LinCombArgs{};
                ob[l].p[0] = (const uint32_t*)lv(G_Z, l);
                ob[l].p[1] = (const uint32_t*)lv(G_W, l, 2);
                ob[l].count = (has_mimc || has_seq) ? 2 : 1;
                ob[l].out = (uint32_t*)lv(G_TMP, l, 1);
                ob[l].n = (uint32_t)n;
                cb[(size_t)12 * l] = nu[6];
                cb[(size_t)12 * l + 1] = nu[7];
                poly::ScanJob &k0 = kj[(size_t)2 * l], &k1 = kj[(size_t)2 * l + 1];
                k0 = poly::ScanJob{};
                k1 = poly::ScanJob{};
                k0.in = lv(G_TMP, l, 0); k0.out = lv(G_TMP, l, 2); k0.n = n; k0.reverse = true; k0.inclusive = false; k0.z = zs[(size_t)2 * l];
                k1.in = lv(G_TMP, l, 1); k1.out = lv(G_R, l); k1.n = n; k1.reverse = true; k1.inclusive = false; k1.z = zs[(size_t)2 * l + 1];
            }
            RC(poly::lincomb_lanes(lane_tab, oa.data(), L, ca.data(), st));
            RC(poly::lincomb_lanes(lane_tab, ob.data(), L, cb.data(), st)); // nu^7 Z (+ nu^8 w_o)
            RC(poly::scan_lanes(1, kj.data(), 2 * L, lane_tab, scratch, st));
            PendingMany P;
            for (int l = 0; l < L; l++) {
                P.scalars.push_back(lv(G_TMP, l, 2));
                P.scalars.push_back(lv(G_R, l));
            }
            RC(commit_many_begin(P));
            RC(commit_many_end(P, out, &tm[1])); // :650-658
        }
        for (int l = 0; l < L; l++) {
            memcpy(lanes[l].proof.PI_Z, out[2 * l], 64);
            memcpy(lanes[l].proof.PI_Z_OMEGA, out[2 * l + 1], 64);
        }
        tm[0] = now_ms() - t0;
        tm[2] = tm[0] - tm[1];
        tm[3] = timing[3];
        return BBGPU_OK;
    }
    // the witness the handle holds, in the own lane
    int construct_proof(uint64_t* proof_out)
    {
        use(own);
        RC(prove(1, nullptr, timing));
        memcpy(proof_out, &lanes[0].proof, sizeof(Proof));
        challenges = lanes[0].ch;
        return BBGPU_OK;
    }
    // bbgpu_plonk_construct_proof_batch*: `count` witnesses in the batch lanes
    int construct_proof_batch(int count, const bbgpu_plonk_witness* W, uint64_t* proofs_out)
    {
        RC(ensure_lanes(count));
        use(batch);
        RC(prove(count, W, batch_timing));
        for (int l = 0; l < count; l++) {
            memcpy(proofs_out + (size_t)l * BBGPU_PLONK_PROOF_WORDS, &lanes[l].proof, sizeof(Proof));
            batch_challenges[l] = lanes[l].ch;
        }
        batch_count = count;
        return BBGPU_OK;
    }
};
constexpr int PlonkProver::lane_group_vectors[PlonkProver::G_COUNT];

std::mutex g_pmu;
std::vector<PlonkProver*> g_provers;

int check_batch_size(const PlonkProver* p, int count)
{
    if ((size_t)count * p->n > ((size_t)1 << 22)) {
        set_error("count %d x n %zu: a batch holds at most 2^22 gates in all (6 GiB of per-lane state)", count, p->n);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}
// argument checks of the batch entry that need no device: the caller's arrays and the size bound
int check_batch_args(const PlonkProver* p, int count, const uint64_t* const* w_l, const uint64_t* const* w_r, const uint64_t* const* w_o, const void* out,
                     const char* out_name = "proofs_out")
{
    if (count < 1 || count > BBGPU_PLONK_MAX_BATCH) {
        set_error("count %d: a batch holds 1..%d proofs", count, BBGPU_PLONK_MAX_BATCH);
        return BBGPU_ERR_ARG;
    }
    if (!w_l || !w_r || !w_o || !out) {
        set_error("null array: %s", !w_l ? "w_l" : !w_r ? "w_r" : !w_o ? "w_o" : out_name);
        return BBGPU_ERR_ARG;
    }
    for (int j = 0; j < count; j++)
        if (!w_l[j] || !w_r[j] || !w_o[j]) {
            set_error("null entry: %s[%d]", !w_l[j] ? "w_l" : !w_r[j] ? "w_r" : "w_o", j);
            return BBGPU_ERR_ARG;
        }
    return p ? check_batch_size(p, count) : BBGPU_OK;
}

// the same for witness descriptors (bbgpu_plonk_witness): `lane` < 0 names the single descriptor of bbgpu_plonk_prover_set_witness_from
int check_witness_desc(const bbgpu_plonk_witness* w, int lane)
{
    char who[32] = "witness";
    if (lane >= 0) snprintf(who, sizeof who, "witness[%d]", lane);
    if (w->form != BBGPU_PLONK_WITNESS_WIRES && w->form != BBGPU_PLONK_WITNESS_VARIABLES) {
        set_error("%s: unknown form %d", who, w->form);
        return BBGPU_ERR_ARG;
    }
    if (w->where != BBGPU_PLONK_WITNESS_HOST && w->where != BBGPU_PLONK_WITNESS_DEVICE) {
        set_error("%s: unknown where %d", who, w->where);
        return BBGPU_ERR_ARG;
    }
    if (w->form == BBGPU_PLONK_WITNESS_WIRES && (!w->w_l || !w->w_r || !w->w_o)) {
        set_error("%s: null pointer: %s", who, !w->w_l ? "w_l" : !w->w_r ? "w_r" : "w_o");
        return BBGPU_ERR_ARG;
    }
    if (w->form == BBGPU_PLONK_WITNESS_VARIABLES && !w->variables) {
        set_error("%s: null pointer: variables", who);
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}
int check_witness_descs(int count, const bbgpu_plonk_witness* w, const void* out, const char* out_name)
{
    if (count < 1 || count > BBGPU_PLONK_MAX_BATCH) {
        set_error("count %d: a batch holds 1..%d proofs", count, BBGPU_PLONK_MAX_BATCH);
        return BBGPU_ERR_ARG;
    }
    if (!w || !out) {
        set_error("null array: %s", !w ? "witness descriptors" : out_name);
        return BBGPU_ERR_ARG;
    }
    for (int j = 0; j < count; j++)
        if (int rc = check_witness_desc(w + j, j)) return rc;
    return BBGPU_OK;
}
// what a descriptor asks of the handle: a wire map for the VARIABLES form
int check_witness_state(const PlonkProver* p, int count, const bbgpu_plonk_witness* w)
{
    for (int j = 0; j < count; j++)
        if (w[j].form == BBGPU_PLONK_WITNESS_VARIABLES && !p->wire_map) {
            set_error("witness in VARIABLES form, but the prover has no wire map: bbgpu_plonk_prover_set_wire_map first");
            return BBGPU_ERR_STATE;
        }
    return BBGPU_OK;
}
// A DEVICE pointer is dereferenced by a kernel: with XNACK off a pointer the device cannot reach faults the card, so everything but device memory of
// the calling thread's current device (context 0's, after bind_calling_thread) is refused here, before anything is enqueued.
int check_device_range(const void* ptr, size_t bytes, const char* who, const char* name)
{
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError(); // (or the next launch check would report it)
        set_error("%s: %s = %p is not memory the HIP runtime knows: where = DEVICE takes device memory", who, name, ptr);
        return BBGPU_ERR_ARG;
    }
    if (a.type != hipMemoryTypeDevice || a.device != dev) {
        set_error("%s: %s = %p is %s, not device memory of device %d (the prover's)", who, name, ptr,
                  a.type == hipMemoryTypeDevice ? "memory of another device" : a.type == hipMemoryTypeHost ? "host memory" : "not plain device memory", dev);
        return BBGPU_ERR_ARG;
    }
    if ((uintptr_t)ptr & 15u) {
        set_error("%s: %s = %p is not 16-byte aligned", who, name, ptr);
        return BBGPU_ERR_ARG;
    }
    void* base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s: %s = %p: the HIP runtime cannot tell the extent of its allocation, so the vector cannot be shown to lie inside it", who, name, ptr);
        return BBGPU_ERR_ARG;
    }
    if ((const char*)ptr + bytes > (const char*)base + size) {
        set_error("%s: %s = %p + %zu bytes runs past the end of its allocation (%p + %zu)", who, name, ptr, bytes, base, size);
        return BBGPU_ERR_ARG;
    }
    return BBGPU_OK;
}
int check_device_pointers(const PlonkProver* p, int count, const bbgpu_plonk_witness* w, bool single = false)
{
    for (int j = 0; j < count; j++) {
        if (w[j].where != BBGPU_PLONK_WITNESS_DEVICE) continue;
        char who[32] = "witness";
        if (!single) snprintf(who, sizeof who, "witness[%d]", j);
        if (w[j].form == BBGPU_PLONK_WITNESS_VARIABLES) {
            RC(check_device_range(w[j].variables, p->num_variables * 32, who, "variables"));
        } else {
            RC(check_device_range(w[j].w_l, p->n * 32, who, "w_l"));
            RC(check_device_range(w[j].w_r, p->n * 32, who, "w_r"));
            RC(check_device_range(w[j].w_o, p->n * 32, who, "w_o"));
        }
    }
    return BBGPU_OK;
}
// the descriptors of the host-array entries
void wires_on_host(int count, const uint64_t* const* w_l, const uint64_t* const* w_r, const uint64_t* const* w_o, bbgpu_plonk_witness* out)
{
    for (int j = 0; j < count; j++) {
        out[j] = bbgpu_plonk_witness{};
        out[j].form = BBGPU_PLONK_WITNESS_WIRES;
        out[j].where = BBGPU_PLONK_WITNESS_HOST;
        out[j].w_l = w_l[j];
        out[j].w_r = w_r[j];
        out[j].w_o = w_o[j];
    }
}

PlonkProver* get(int h)
{
    if (h < 0 || h >= (int)g_provers.size() || !g_provers[h]) {
        set_error("unknown prover handle %d", h);
        return nullptr;
    }
    return g_provers[h];
}

} // namespace

std::mutex& plonk_mutex() { return g_pmu; }
uint64_t plonk_lane_bytes() { return g_lane_bytes.load(); }
void plonk_release_all_locked()
{
    for (auto*& p : g_provers) {
        delete p;
        p = nullptr;
    }
    g_provers.clear();
    for (hipStream_t q : g_idle_streams) (void)hipStreamDestroy(q);
    g_idle_streams.clear();
}

} // namespace bbgpu

using namespace bbgpu;

#pragma GCC visibility push(default)
extern "C" {

// what can be said about a circuit description without a device (bbgpu_plonk_prover_create, bbgpu_host_plonk_check_witness)
static int check_circuit_fields(const bbgpu_plonk_circuit* c)
{
    if (!c || !c->w_l || !c->w_r || !c->w_o || !c->sigma_1_mapping || !c->sigma_2_mapping || !c->sigma_3_mapping || !c->q_m || !c->q_l || !c->q_r ||
        !c->q_o || !c->q_c) {
        set_error("null circuit field");
        return BBGPU_ERR_ARG;
    }
    if ((c->q_bl != nullptr) != (c->q_br != nullptr) || (c->q_bl != nullptr) != (c->q_bo != nullptr)) {
        set_error("bool widget selectors: give all of q_bl, q_br, q_bo or none");
        return BBGPU_ERR_ARG;
    }
    if ((c->q_mimc_selector != nullptr) != (c->q_mimc_coefficient != nullptr) || (c->q_mimc_selector && (c->q_bl || c->q_o_next))) {
        set_error("MiMC widget selectors: give both q_mimc_selector and q_mimc_coefficient or neither, and not together with the bool or the sequential widget");
        return BBGPU_ERR_ARG;
    }
    // 2^21: the largest circuit with a REFERENCE proof to compare against (tests/golden/plonk_proofs.json); nothing in the kernels stops there any more -- the
    // scans nest to 2^28 elements (poly.hip, round 4), the transforms reach 2^28, the commitments run over table segments -- but a proof of a larger circuit
    // would be parity-unpinned, so the entry refuses it instead of returning bytes no reference ever produced.
    if (c->n < 4 || (c->n & (c->n - 1)) || c->n > ((size_t)1 << 21)) {
        set_error("circuit size %zu: must be a power of two, 4 <= n <= 2^21 (the largest size a reference proof exists for: larger proofs would be parity-unpinned)", c->n);
        return BBGPU_ERR_SIZE;
    }
    return BBGPU_OK;
}

int bbgpu_plonk_prover_create(const bbgpu_plonk_circuit* c, int srs_handle)
{
    if (int rc = check_circuit_fields(c)) return rc;
    const int W = bbgpu_srs_num_windows(srs_handle, c->n);
    if (W < 0) {
        set_error("unknown SRS handle %d", srs_handle);
        return BBGPU_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(g_pmu);
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    PlonkProver* p = new PlonkProver();
    int rc = p->init(c, srs_handle);
    if (rc) {
        delete p;
        return rc;
    }
    g_provers.push_back(p);
    return (int)g_provers.size() - 1;
}

int bbgpu_plonk_prover_set_witness(int prover, const uint64_t* w_l, const uint64_t* w_r, const uint64_t* w_o)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    PlonkProver* p = get(prover);
    if (!p || !w_l || !w_r || !w_o) return BBGPU_ERR_ARG;
    bbgpu_plonk_witness W;
    wires_on_host(1, &w_l, &w_r, &w_o, &W);
    const int rc = p->set_witness_from(W);
    if (rc) (void)hipStreamSynchronize(p->st); // the caller's arrays are no longer read when it sees the error
    return rc;
}

int bbgpu_plonk_construct_proof(int prover, uint64_t proof_out[BBGPU_PLONK_PROOF_WORDS])
{
    std::lock_guard<std::mutex> lk(g_pmu);
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    PlonkProver* p = get(prover);
    if (!p || !proof_out) return BBGPU_ERR_ARG;
    const int rc = p->construct_proof(proof_out);
    if (rc) (void)hipStreamSynchronize(p->st); // nothing of a failed proof is still running when the caller sees the error
    return rc;
}

int bbgpu_plonk_construct_proof_batch(int prover, int count, const uint64_t* const* w_l, const uint64_t* const* w_r, const uint64_t* const* w_o,
                                      uint64_t* proofs_out)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    // everything that can be refused without a device is refused before one is bound
    if (int rc = check_batch_args(nullptr, count, w_l, w_r, w_o, proofs_out)) return rc;
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    if (int rc = check_batch_args(p, count, w_l, w_r, w_o, proofs_out)) return rc;
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    bbgpu_plonk_witness W[BBGPU_PLONK_MAX_BATCH];
    wires_on_host(count, w_l, w_r, w_o, W);
    const int rc = p->construct_proof_batch(count, W, proofs_out);
    if (rc) (void)hipStreamSynchronize(p->st); // nothing of a failed batch is still running when the caller sees the error
    return rc;
}

int bbgpu_plonk_prover_set_wire_map(int prover, const uint32_t* w_l_index, const uint32_t* w_r_index, const uint32_t* w_o_index, size_t num_variables)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    // everything that can be refused without a device is refused before one is bound
    if (!w_l_index || !w_r_index || !w_o_index) {
        set_error("null array: %s", !w_l_index ? "w_l_index" : !w_r_index ? "w_r_index" : "w_o_index");
        return BBGPU_ERR_ARG;
    }
    if (num_variables == 0) {
        set_error("num_variables 0: a wire map references at least one variable");
        return BBGPU_ERR_SIZE;
    }
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    if (num_variables > 4 * p->n) {
        set_error("num_variables %zu: at most 4 n = %zu (a map of n = %zu gates references at most 3 n variables)", num_variables, 4 * p->n, p->n);
        return BBGPU_ERR_SIZE;
    }
    const uint32_t* const idx[3] = { w_l_index, w_r_index, w_o_index };
    static const char* const names[3] = { "w_l_index", "w_r_index", "w_o_index" };
    for (int k = 0; k < 3; k++)
        for (size_t i = 0; i < p->n; i++)
            if (idx[k][i] >= num_variables) {
                set_error("%s[%zu] = %u is not below num_variables %zu", names[k], i, idx[k][i], num_variables);
                return BBGPU_ERR_ARG;
            }
    if (int rcb = bind_calling_thread()) return rcb; // the copies below are enqueued from THIS thread
    return p->set_wire_map(idx, num_variables);
}

int bbgpu_plonk_prover_set_witness_from(int prover, const bbgpu_plonk_witness* w)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    if (!w) {
        set_error("null witness descriptor");
        return BBGPU_ERR_ARG;
    }
    if (int rc = check_witness_desc(w, -1)) return rc;
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    if (int rc = check_witness_state(p, 1, w)) return rc;
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    if (int rc = check_device_pointers(p, 1, w, true)) return rc;
    const int rc = p->set_witness_from(*w);
    if (rc) (void)hipStreamSynchronize(p->st); // the caller's buffers are no longer read when it sees the error
    return rc;
}

int bbgpu_plonk_construct_proof_batch_from(int prover, int count, const bbgpu_plonk_witness* w, uint64_t* proofs_out)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    // everything that can be refused without a device is refused before one is bound
    if (int rc = check_witness_descs(count, w, proofs_out, "proofs_out")) return rc;
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    if (int rc = check_batch_size(p, count)) return rc;
    if (int rc = check_witness_state(p, count, w)) return rc;
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    if (int rc = check_device_pointers(p, count, w)) return rc;
    const int rc = p->construct_proof_batch(count, w, proofs_out);
    if (rc) (void)hipStreamSynchronize(p->st); // nothing of a failed batch is still running when the caller sees the error
    return rc;
}

int bbgpu_plonk_check_witness_batch_from(int prover, int count, const bbgpu_plonk_witness* w, bbgpu_plonk_witness_report* out)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    // everything that can be refused without a device is refused before one is bound
    if (int rc = check_witness_descs(count, w, out, "out")) return rc;
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    if (int rc = check_batch_size(p, count)) return rc;
    if (int rc = check_witness_state(p, count, w)) return rc;
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    if (int rc = check_device_pointers(p, count, w)) return rc;
    const int rc = p->check_witness_batch(count, w, out);
    if (rc) (void)hipStreamSynchronize(p->st); // the caller's buffers are no longer read when it sees the error
    return rc;
}

int bbgpu_plonk_check_witness(int prover, bbgpu_plonk_witness_report* out)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p || !out) return BBGPU_ERR_ARG;
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    const int rc = p->check_witness(out);
    if (rc) (void)hipStreamSynchronize(p->st);
    return rc;
}

int bbgpu_plonk_check_witness_batch(int prover, int count, const uint64_t* const* w_l, const uint64_t* const* w_r, const uint64_t* const* w_o,
                                    bbgpu_plonk_witness_report* out)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    // everything that can be refused without a device is refused before one is bound
    if (int rc = check_batch_args(nullptr, count, w_l, w_r, w_o, out, "out")) return rc;
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    if (int rc = check_batch_args(p, count, w_l, w_r, w_o, out, "out")) return rc;
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    bbgpu_plonk_witness W[BBGPU_PLONK_MAX_BATCH];
    wires_on_host(count, w_l, w_r, w_o, W);
    const int rc = p->check_witness_batch(count, W, out);
    if (rc) (void)hipStreamSynchronize(p->st); // the caller's arrays are no longer read when it sees the error
    return rc;
}

int bbgpu_plonk_set_witness_check(int prover, int enabled)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    p->witness_check = enabled != 0;
    return BBGPU_OK;
}

int bbgpu_plonk_last_witness_report(int prover, int lane, bbgpu_plonk_witness_report* out)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p || !out) return BBGPU_ERR_ARG;
    if (lane < 0 || lane >= p->report_count) {
        set_error("lane %d: the last witness check of this prover covered %d", lane, p->report_count);
        return BBGPU_ERR_ARG;
    }
    *out = p->reports[lane];
    return BBGPU_OK;
}

// the same definition on the host (host_plonk_check.hpp): no HIP call, no lock, no state
int bbgpu_host_plonk_check_witness(const bbgpu_plonk_circuit* circuit, bbgpu_plonk_witness_report* out)
{
    if (int rc = check_circuit_fields(circuit)) return rc;
    if (!out) {
        set_error("null report");
        return BBGPU_ERR_ARG;
    }
    *out = host::plonk_check_witness(*circuit);
    return BBGPU_OK;
}

int bbgpu_plonk_batch_challenges(int prover, int lane, uint64_t out[20])
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p || !out) return BBGPU_ERR_ARG;
    if (lane < 0 || lane >= p->batch_count) {
        set_error("lane %d: the last batch of this prover had %d", lane, p->batch_count);
        return BBGPU_ERR_ARG;
    }
    memcpy(out, &p->batch_challenges[lane], 160);
    return BBGPU_OK;
}

int bbgpu_plonk_last_batch_timing(int prover, double ms_out[4])
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p || !ms_out) return BBGPU_ERR_ARG;
    for (int i = 0; i < 4; i++) ms_out[i] = p->batch_timing[i];
    return BBGPU_OK;
}

int bbgpu_plonk_preprocess(int prover, uint64_t vk_out[BBGPU_PLONK_VK_WORDS])
{
    std::lock_guard<std::mutex> lk(g_pmu);
    if (int rcb = bind_calling_thread()) return rcb; // the kernels below are launched from THIS thread
    PlonkProver* p = get(prover);
    if (!p || !vk_out) return BBGPU_ERR_ARG;
    return p->preprocess(reinterpret_cast<uint64_t(*)[8]>(vk_out));
}

int bbgpu_plonk_last_challenges(int prover, uint64_t out[20])
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p || !out) return BBGPU_ERR_ARG;
    memcpy(out, &p->challenges, 160);
    return BBGPU_OK;
}

int bbgpu_plonk_last_timing(int prover, double ms_out[4])
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p || !ms_out) return BBGPU_ERR_ARG;
    for (int i = 0; i < 4; i++) ms_out[i] = p->timing[i];
    return BBGPU_OK;
}

// challenge.hpp:64-112 on a finished proof: gamma, beta, alpha and the evaluation challenge z (what a verifier recomputes).
// Host arithmetic only; needs no GPU.
int bbgpu_plonk_challenges_from_proof(const uint64_t proof_words[BBGPU_PLONK_PROOF_WORDS], uint64_t out[16])
{
    if (!proof_words || !out) return BBGPU_ERR_ARG;
    Proof proof;
    memcpy(&proof, proof_words, sizeof(Proof));
    std::vector<uint64_t> b = PlonkProver::transcript_of(proof, 0);
    const Fr gamma = PlonkProver::challenge(b);
    PlonkProver::put_fr(b, gamma);
    const Fr beta = PlonkProver::challenge(b);
    const Fr alpha = PlonkProver::challenge(PlonkProver::transcript_of(proof, 1));
    const Fr z = PlonkProver::challenge(PlonkProver::transcript_of(proof, 2));
    memcpy(out, gamma.d, 32);
    memcpy(out + 4, beta.d, 32);
    memcpy(out + 8, alpha.d, 32);
    memcpy(out + 12, z.d, 32);
    return BBGPU_OK;
}

int bbgpu_plonk_prover_destroy(int prover)
{
    std::lock_guard<std::mutex> lk(g_pmu);
    PlonkProver* p = get(prover);
    if (!p) return BBGPU_ERR_ARG;
    delete p;
    g_provers[prover] = nullptr;
    return BBGPU_OK;
}

} // extern "C"
#pragma GCC visibility pop
