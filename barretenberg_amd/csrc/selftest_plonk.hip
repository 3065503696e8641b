// selftest_plonk.hip -- bbgpu_selftest_plonk_round (include/bbgpu.h): ONE round kernel of the PLONK prover on caller-given vectors and challenges, so that
// each of them is pinned against a plain statement of its formula (tests/plonk_round_cases.py) and not only through the bytes of whole proofs, whose
// circuits never carry a live q_c or q_bo, a full-width selector, an operand above 2r or lanes that differ.  Nothing of the kernels is restated here: the
// entry uploads the vectors, writes one argument record per lane with device pointers into them and calls the host function plonk.hip calls (poly.h) with a
// LaneTable and a Scratch of its own -- the records' constants, the grids and the launches are the product's.  Host pointers in and out, as in selftest.hip.
#include <hip/hip_runtime.h>

#include <string.h>
#include <vector>

#include "bbgpu_internal.h"
#include "host_fr.hpp"
#include "poly.h"

namespace bbgpu {
namespace {

using host::Fr;

constexpr int MAX_IN = 13, MAX_OUT = 2, MAX_LANES = 16;
constexpr size_t MAX_ELEMS = (size_t)1 << 22; // lanes x the longest vector of a call (128 MiB); also scan_lanes' own limit for one job

// what a call moves: per-lane element counts of its vectors (bbgpu.h has the table)
struct Shape {
    int num_in = 0, num_out = 0;
    size_t in_len[MAX_IN] = {}, out_len[MAX_OUT] = {};
    int out_from[MAX_OUT] = { -1, -1 }; // the input whose device buffer IS this output (in place), or -1: a fresh buffer, preset to all-ones
    size_t consts = 0;                  // in all
    void in(int count, size_t len) { for (int k = 0; k < count; k++) in_len[num_in++] = len; }
    void fresh(size_t len) { out_len[num_out++] = len; }
    void in_place(int from) { out_from[num_out] = from; out_len[num_out++] = in_len[from]; }
};

bool pow2(size_t v) { return v && !(v & (v - 1)); }
int log2_of(size_t v) { int l = 0; while (((size_t)1 << l) < v) l++; return l; }
bool below_r(const uint64_t* v)
{
    for (int i = 3; i >= 0; i--)
        if (v[i] != FrHostP::P[i]) return v[i] < FrHostP::P[i];
    return false;
}

// BBGPU_OK and the shape, or BBGPU_ERR_ARG for what the kernel behind `kernel` does not support.  Host arithmetic only.
int shape_of(int kernel, int lanes, size_t len, const uint32_t* params, int num_params, Shape& S)
{
    if (lanes < 1 || lanes > MAX_LANES || len == 0 || len > MAX_ELEMS || num_params < 0 || (num_params && !params)) return BBGPU_ERR_ARG;
    const size_t L = (size_t)lanes;
    int want_params = 0;
    switch (kernel) {
    case BBGPU_SELFTEST_PLONK_Z_TERMS: // w^i from a table of the 2^k-th root: a power of two
        if (!pow2(len)) return BBGPU_ERR_ARG;
        S.in(6, len); S.fresh(len); S.fresh(len); S.consts = 2 * L;
        break;
    case BBGPU_SELFTEST_PLONK_QUOT_LARGE: // index i + 4 is masked with 4n - 1
        if (!pow2(len) || len < 4) return BBGPU_ERR_ARG;
        S.in(7, len); S.fresh(len); S.consts = 2 * L;
        break;
    case BBGPU_SELFTEST_PLONK_QUOT_MID: // 2i + 4 masked with 4n - 1, i + 4 with 2n - 1
        if (!pow2(len) || len < 2) return BBGPU_ERR_ARG;
        S.in(4, 2 * len); S.in(6, len); S.fresh(len); S.consts = 2 * L;
        break;
    case BBGPU_SELFTEST_PLONK_QUOT_SEQ:
        if (!pow2(len) || len < 2) return BBGPU_ERR_ARG;
        S.in(1, 2 * len); S.in(2, len); S.in_place(2); S.consts = L;
        break;
    case BBGPU_SELFTEST_PLONK_QUOT_BOOL:
        if (!pow2(len) || len < 2) return BBGPU_ERR_ARG;
        S.in(3, 2 * len); S.in(4, len); S.in_place(6); S.consts = 3 * L;
        break;
    case BBGPU_SELFTEST_PLONK_QUOT_MIMC:
        if (!pow2(len) || len < 4) return BBGPU_ERR_ARG;
        S.in(6, len); S.in_place(5); S.consts = 2 * L;
        break;
    case BBGPU_SELFTEST_PLONK_LINCOMB:
        want_params = 2;
        if (num_params != 2 || params[0] < 1 || params[0] > 12 || params[1] > 1) return BBGPU_ERR_ARG;
        S.in((int)(params[0] + params[1]), len); S.fresh(len); S.consts = params[0] * L;
        break;
    case BBGPU_SELFTEST_PLONK_MUL2C:
        S.in(2, len); S.fresh(len); S.consts = L;
        break;
    case BBGPU_SELFTEST_PLONK_SIGMA_PREPARE:
        want_params = 1;
        if (num_params != 1 || params[0] < len) return BBGPU_ERR_ARG;
        S.in(2, len); S.fresh(params[0]); S.consts = L;
        break;
    case BBGPU_SELFTEST_PLONK_COPY_PAD:
        want_params = 2;
        if (num_params != 2 || params[0] < len || params[1] > 1) return BBGPU_ERR_ARG;
        S.in(1, len); S.fresh(params[0]); S.consts = params[1] ? L : 0;
        break;
    case BBGPU_SELFTEST_PLONK_ADD_INPLACE: // lane l of a vector at base + l * stride
        want_params = 2;
        if (num_params != 2 || params[0] < len || params[1] < len) return BBGPU_ERR_ARG;
        S.in(1, params[0]); S.in(1, params[1]); S.in_place(0);
        break;
    case BBGPU_SELFTEST_PLONK_DIVIDE_VANISHING: // N = 2^k, n = N / 1, 2 or 4
        want_params = 2;
        if (num_params != 2 || !pow2(len) || params[0] > 2 || len < ((size_t)1 << params[0]) || params[1] < len) return BBGPU_ERR_ARG;
        S.in(1, params[1]); S.in_place(0);
        break;
    case BBGPU_SELFTEST_PLONK_SCAN:
        want_params = 2;
        if (num_params != 2 || params[0] > 1 || params[1] > 15 || !(params[1] & 12)) return BBGPU_ERR_ARG;
        S.in(1, len);
        if (params[1] & 4) S.fresh(len);
        if (params[1] & 8) S.fresh(1);
        S.consts = params[0] ? L : 0;
        break;
    case BBGPU_SELFTEST_PLONK_EVALUATE:
        want_params = 1 + lanes;
        if (num_params != want_params || params[0] < 1 || params[0] > 16) return BBGPU_ERR_ARG;
        for (int j = 0; j < lanes; j++)
            if (params[1 + j] >= params[0]) return BBGPU_ERR_ARG;
        S.in(1, len); S.fresh(1); S.consts = params[0];
        break;
    default: return BBGPU_ERR_ARG;
    }
    if (num_params != want_params) return BBGPU_ERR_ARG;
    for (int i = 0; i < S.num_in; i++)
        if (S.in_len[i] > MAX_ELEMS / L) return BBGPU_ERR_ARG;
    for (int o = 0; o < S.num_out; o++)
        if (S.out_len[o] > MAX_ELEMS / L) return BBGPU_ERR_ARG;
    return BBGPU_OK;
}

// everything the call holds on the device, released on every way out
struct Held {
    uint64_t* d_in[MAX_IN] = {};
    uint64_t* d_fresh[MAX_OUT] = {};
    poly::LaneTable tab;
    poly::Scratch scratch;
    ~Held()
    {
        for (uint64_t* p : d_in)
            if (p) (void)hipFree(p);
        for (uint64_t* p : d_fresh)
            if (p) (void)hipFree(p);
        tab.release();
        scratch.release();
    }
};

#define HIPOK(x)                                                                                                                                        \
    do {                                                                                                                                                \
        hipError_t e_ = (x);                                                                                                                            \
        if (e_ != hipSuccess) {                                                                                                                         \
            set_error("selftest_plonk_round: %s -> %s", #x, hipGetErrorString(e_));                                                                     \
            return BBGPU_ERR_HIP;                                                                                                                       \
        }                                                                                                                                               \
    } while (0)

// lane l of a lane-major device vector, as the kernels' word pointer
const uint32_t* at(const uint64_t* base, size_t per_lane, int l) { return (const uint32_t*)(base + (size_t)l * per_lane * 4); }
uint32_t* at(uint64_t* base, size_t per_lane, int l) { return (uint32_t*)(base + (size_t)l * per_lane * 4); }

int launch(int kernel, int lanes, size_t len, const uint32_t* params, const Shape& S, Held& H, uint64_t* const* d_out, const std::vector<Fr>& c)
{
    hipStream_t st = nullptr;
    const uint32_t n = (uint32_t)len;
    uint64_t* const* I = H.d_in;
    // constant k of lane l (lane-major), gathered into one array per constant as the host functions take them
    auto column = [&](int k, int per_lane) {
        std::vector<Fr> v((size_t)lanes);
        for (int l = 0; l < lanes; l++) v[l] = c[(size_t)l * per_lane + k];
        return v;
    };
    switch (kernel) {
    case BBGPU_SELFTEST_PLONK_Z_TERMS: {
        std::vector<poly::ZTermsArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::ZTermsArgs{};
            A[l].w_l = at(I[0], len, l); A[l].w_r = at(I[1], len, l); A[l].w_o = at(I[2], len, l);
            A[l].s1 = at(I[3], len, l); A[l].s2 = at(I[4], len, l); A[l].s3 = at(I[5], len, l);
            A[l].num = at(d_out[0], len, l); A[l].den = at(d_out[1], len, l);
            A[l].n = n;
        }
        const std::vector<Fr> beta = column(0, 2), gamma = column(1, 2);
        return poly::z_terms_lanes(H.tab, A.data(), lanes, host::fr_root_of_unity(log2_of(len)), beta.data(), gamma.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_QUOT_LARGE: {
        std::vector<poly::QuotLargeArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::QuotLargeArgs{};
            A[l].wl_f = at(I[0], len, l); A[l].wr_f = at(I[1], len, l); A[l].wo_f = at(I[2], len, l);
            A[l].s1_f = at(I[3], len, l); A[l].s2_f = at(I[4], len, l); A[l].s3_f = at(I[5], len, l);
            A[l].z_f = at(I[6], len, l);
            A[l].q = at(d_out[0], len, l);
            A[l].n4 = n;
        }
        const std::vector<Fr> beta = column(0, 2), gamma = column(1, 2);
        return poly::quotient_large_lanes(H.tab, A.data(), lanes, host::fr_root_of_unity(log2_of(len)), beta.data(), gamma.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_QUOT_MID: {
        std::vector<poly::QuotMidArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::QuotMidArgs{};
            A[l].z_f = at(I[0], 2 * len, l); A[l].wl_f = at(I[1], 2 * len, l); A[l].wr_f = at(I[2], 2 * len, l); A[l].wo_f = at(I[3], 2 * len, l);
            A[l].l1 = at(I[4], len, l);
            A[l].qm_f = at(I[5], len, l); A[l].ql_f = at(I[6], len, l); A[l].qr_f = at(I[7], len, l); A[l].qo_f = at(I[8], len, l);
            A[l].qc_f = at(I[9], len, l);
            A[l].q = at(d_out[0], len, l);
            A[l].n2 = n;
        }
        const std::vector<Fr> alpha = column(0, 2), abase = column(1, 2);
        return poly::quotient_mid_lanes(H.tab, A.data(), lanes, alpha.data(), abase.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_QUOT_SEQ: {
        std::vector<poly::QuotSeqArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::QuotSeqArgs{};
            A[l].wo_f = at(I[0], 2 * len, l);
            A[l].qon_f = at(I[1], len, l);
            A[l].q = at(d_out[0], len, l);
            A[l].n2 = n;
        }
        return poly::quotient_seq_lanes(H.tab, A.data(), lanes, c.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_QUOT_BOOL: {
        std::vector<poly::QuotBoolArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::QuotBoolArgs{};
            A[l].wl_f = at(I[0], 2 * len, l); A[l].wr_f = at(I[1], 2 * len, l); A[l].wo_f = at(I[2], 2 * len, l);
            A[l].qbl_f = at(I[3], len, l); A[l].qbr_f = at(I[4], len, l); A[l].qbo_f = at(I[5], len, l);
            A[l].q = at(d_out[0], len, l);
            A[l].n2 = n;
        }
        const std::vector<Fr> cl = column(0, 3), cr = column(1, 3), co = column(2, 3);
        return poly::quotient_bool_lanes(H.tab, A.data(), lanes, cl.data(), cr.data(), co.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_QUOT_MIMC: {
        std::vector<poly::QuotMimcArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::QuotMimcArgs{};
            A[l].wl_f = at(I[0], len, l); A[l].wr_f = at(I[1], len, l); A[l].wo_f = at(I[2], len, l);
            A[l].qsel_f = at(I[3], len, l); A[l].qcoef_f = at(I[4], len, l);
            A[l].q = at(d_out[0], len, l);
            A[l].n4 = n;
        }
        const std::vector<Fr> abase = column(0, 2), astep = column(1, 2);
        return poly::quotient_mimc_lanes(H.tab, A.data(), lanes, abase.data(), astep.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_LINCOMB: {
        const int count = (int)params[0];
        std::vector<poly::LinCombArgs> A((size_t)lanes);
        std::vector<Fr> coeffs((size_t)lanes * 12, host::fr_zero());
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::LinCombArgs{};
            for (int j = 0; j < count; j++) {
                A[l].p[j] = at(I[j], len, l);
                coeffs[(size_t)l * 12 + j] = c[(size_t)l * count + j];
            }
            A[l].out_add = params[1] ? at(I[count], len, l) : nullptr;
            A[l].out = at(d_out[0], len, l);
            A[l].n = n;
            A[l].count = count;
        }
        return poly::lincomb_lanes(H.tab, A.data(), lanes, coeffs.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_MUL2C: {
        std::vector<poly::Mul2cArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::Mul2cArgs{};
            A[l].a = at(I[0], len, l); A[l].b = at(I[1], len, l);
            A[l].out = at(d_out[0], len, l);
            A[l].n = n;
        }
        return poly::mul2c_lanes(H.tab, A.data(), lanes, c.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_SIGMA_PREPARE: {
        std::vector<poly::SigmaPrepArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::SigmaPrepArgs{};
            A[l].sigma = at(I[0], len, l); A[l].w = at(I[1], len, l);
            A[l].dst = at(d_out[0], S.out_len[0], l);
            A[l].n = n;
            A[l].n_dst = params[0];
        }
        return poly::sigma_prepare_lanes(H.tab, A.data(), lanes, c.data(), st);
    }
    case BBGPU_SELFTEST_PLONK_COPY_PAD: {
        std::vector<poly::CopyPadArgs> A((size_t)lanes);
        for (int l = 0; l < lanes; l++) {
            A[l] = poly::CopyPadArgs{};
            A[l].src = at(I[0], len, l);
            A[l].dst = at(d_out[0], S.out_len[0], l);
            A[l].n_src = n;
            A[l].n_dst = params[0];
        }
        return poly::copy_pad_lanes(H.tab, A.data(), lanes, params[1] ? c.data() : nullptr, st);
    }
    case BBGPU_SELFTEST_PLONK_ADD_INPLACE:
        return poly::add_inplace_lanes(I[0], params[0], I[1], params[1], len, lanes, st);
    case BBGPU_SELFTEST_PLONK_DIVIDE_VANISHING: {
        const int log2N = log2_of(len);
        return poly::divide_by_pseudo_vanishing_lanes(I[0], params[1], lanes, log2N - (int)params[0], log2N, st);
    }
    case BBGPU_SELFTEST_PLONK_SCAN: {
        const uint32_t flags = params[1];
        uint64_t* d_vec = (flags & 4) ? d_out[0] : nullptr;
        uint64_t* d_tot = (flags & 8) ? d_out[(flags & 4) ? 1 : 0] : nullptr;
        std::vector<poly::ScanJob> J((size_t)lanes);
        for (int j = 0; j < lanes; j++) {
            J[j] = poly::ScanJob{};
            J[j].in = I[0] + (size_t)j * len * 4;
            J[j].out = d_vec ? d_vec + (size_t)j * len * 4 : nullptr;
            J[j].n = len;
            J[j].reverse = (flags & 1) != 0;
            J[j].inclusive = (flags & 2) != 0;
            if (params[0]) J[j].z = c[j];
            J[j].d_total = d_tot ? d_tot + (size_t)j * 4 : nullptr;
        }
        return poly::scan_lanes((int)params[0], J.data(), lanes, H.tab, H.scratch, st);
    }
    case BBGPU_SELFTEST_PLONK_EVALUATE: {
        std::vector<poly::EvalJob> J((size_t)lanes);
        std::vector<int> zidx((size_t)lanes);
        for (int j = 0; j < lanes; j++) {
            J[j] = poly::EvalJob{};
            J[j].coeffs = I[0] + (size_t)j * len * 4;
            J[j].n = len;
            J[j].zsel = (int)params[1 + j];
            J[j].d_result = d_out[0] + (size_t)j * 4;
            zidx[j] = (int)params[1 + j];
        }
        return poly::evaluate_lanes(J.data(), zidx.data(), lanes, c.data(), (int)params[0], H.tab, H.scratch, st);
    }
    }
    return BBGPU_ERR_ARG;
}

} // namespace
} // namespace bbgpu

using namespace bbgpu;

#pragma GCC visibility push(default)
extern "C" {

int bbgpu_selftest_plonk_round(int kernel, int lanes, size_t len, const uint32_t* params, int num_params, const uint64_t* const* in, int num_in,
                               const uint64_t* consts, size_t num_consts, uint64_t* const* out, int num_out)
{
    Shape S;
    std::vector<Fr> c;
    const bool ok = [&] {
        if (shape_of(kernel, lanes, len, params, num_params, S) != BBGPU_OK) return false;
        if (num_in != S.num_in || num_out != S.num_out || num_consts != S.consts || !in || !out || (S.consts && !consts)) return false;
        for (int i = 0; i < S.num_in; i++)
            if (!in[i]) return false;
        for (int o = 0; o < S.num_out; o++)
            if (!out[o]) return false;
        c.resize(S.consts);
        for (size_t k = 0; k < S.consts; k++) {
            if (!below_r(consts + 4 * k)) return false; // a challenge is a reduced value: the records' constants are made from canonical ones
            memcpy(c[k].d, consts + 4 * k, 32);
        }
        return true;
    }();
    if (!ok) {
        set_error("selftest_plonk_round: kernel %d with %d lanes of %zu elements, %d parameters, %d + %d vectors, %zu constants: not supported (include/bbgpu.h)",
                  kernel, lanes, len, num_params, num_in, num_out, num_consts);
        return BBGPU_ERR_ARG;
    }
    if (bbgpu_device_count() == 0) {
        set_error("no HIP device available: libbbgpu has no CPU fallback");
        return BBGPU_ERR_HIP;
    }
    Held H;
    uint64_t* d_out[MAX_OUT] = {};
    const size_t L = (size_t)lanes;
    for (int i = 0; i < S.num_in; i++) {
        HIPOK(hipMalloc((void**)&H.d_in[i], L * S.in_len[i] * 32));
        HIPOK(hipMemcpy(H.d_in[i], in[i], L * S.in_len[i] * 32, hipMemcpyHostToDevice));
    }
    for (int o = 0; o < S.num_out; o++) {
        if (S.out_from[o] >= 0) {
            d_out[o] = H.d_in[S.out_from[o]];
            continue;
        }
        HIPOK(hipMalloc((void**)&H.d_fresh[o], L * S.out_len[o] * 32));
        HIPOK(hipMemset(H.d_fresh[o], 0xff, L * S.out_len[o] * 32));
        d_out[o] = H.d_fresh[o];
    }
    if (int rc = H.tab.init((size_t)1 << 20)) return rc;
    if (int rc = launch(kernel, lanes, len, params, S, H, d_out, c)) return rc;
    HIPOK(hipDeviceSynchronize());
    for (int o = 0; o < S.num_out; o++) HIPOK(hipMemcpy(out[o], d_out[o], L * S.out_len[o] * 32, hipMemcpyDeviceToHost));
    return BBGPU_OK;
}

} // extern "C"
#pragma GCC visibility pop
