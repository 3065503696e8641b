// srs_lagrange.hip -- the device part of bbgpu_srs_lagrange (include/bbgpu.h): rows [0, n) of a resident table, P_j, become the same string in the Lagrange
// basis of the size-n domain, L_i = n^-1 sum_j omega^(-i j) P_j: an inverse NTT whose elements are curve points.  Radix-2, decimation in time, one lane per
// butterfly, on a scratch of n projective points (XYZZ, 128 bytes each; g1_ladder.hpp):
//   k_lagrange_load    slot i <- n^-1 * P_bitrev(i): the scaling goes in here, one ladder per row over an affine base, no inversion;
//   k_lagrange_stage   (g1_stage.hpp) log2 n launches, in place: (a, b) -> (a + w b, a - w b) with w = omega^(-e) made in the lane by square-and-multiply on e (as
//                      k_srs_update makes y^e; no twiddle table) and w b by the ladder of k_srs_update over a projective base.  e == 0 skips the ladder;
//   k_lagrange_finish  one Fermat inversion per row to the resident form; rows at infinity are counted as k_srs_on_curve counts its findings.
// The reference has no counterpart: its strings are monomial (io.hpp:159-181) and its Lagrange-basis polynomials are transformed, never committed as values.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "g1_stage.hpp"

namespace bbgpu {

namespace {

constexpr int FT = 256; // threads per workgroup of the finish kernel, as k_srs_on_curve (LT, of the ladder kernels, and the windows: g1_stage.hpp)

struct Scalar256 {
    uint64_t d[4];
};

// slot i <- k * row bitrev(i), k = n^-1 as a plain integer (the same in every lane)
__global__ void __launch_bounds__(LT) k_lagrange_load(const uint32_t* __restrict__ in, uint32_t* __restrict__ scratch, uint32_t n, uint32_t log2n, Scalar256 k)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = __brev(i) >> (32 - log2n); // log2n >= 1; j < n
    uint32_t w[16];
    const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)j * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint4 v = src[t];
        w[4 * t] = v.x; w[4 * t + 1] = v.y; w[4 * t + 2] = v.z; w[4 * t + 3] = v.w;
    }
    Pt acc;
    bool inf;
    ladder_pt<LAGRANGE_WB>(w, k.d, acc, inf);
    uint32_t o[32];
    store_pt(o, acc, inf);
    store_words32(scratch + (size_t)i * 32, o);
}

// row i <- the affine form of slot i (Montgomery-261, canonical); a slot at infinity gives a zero row and a finding.  Findings meet on chip as in
// k_srs_on_curve: shuffles inside a wave, an LDS slot per wave, then ONE thread per workgroup issues the count atomicAdd and the first-row atomicMin, only
// if the workgroup found anything -- an honest table issues no atomic, and sums and minima do not depend on arrival order.
__global__ void __launch_bounds__(FT) k_lagrange_finish(const uint32_t* __restrict__ scratch, uint32_t* __restrict__ rows, uint64_t n, SrsCurveFindings* __restrict__ out)
{
    __shared__ unsigned long long s_first[FT / 64];
    __shared__ uint32_t s_bad[FT / 64];
    const uint64_t nt = (uint64_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    unsigned long long first = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nt) {
        uint32_t w[32], o[16];
        load_words32(scratch + i * 32, w);
        Pt p;
        bool inf;
        load_pt(p, inf, w);
        if (inf) {
            bad++;
            first = i < first ? i : first;
#pragma unroll
            for (int t = 0; t < 16; t++) o[t] = 0;
        } else {
            const auto inv = fq_inverse_fermat(mul(p.zz, p.zzz));
            const auto izz = mul(inv, p.zzz), izzz = mul(inv, p.zz);
            store_affine_m261(o, mul(p.x, izz), mul(p.y, izzz));
        }
        uint4* dst = reinterpret_cast<uint4*>(rows + i * 16);
#pragma unroll
        for (int t = 0; t < 4; t++) dst[t] = make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
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
    for (int k = 1; k < FT / 64; k++) {
        bad += s_bad[k];
        first = s_first[k] < first ? s_first[k] : first;
    }
    if (!bad) return;
    atomicAdd(&out->bad_points, (unsigned long long)bad);
    atomicMin(&out->first_bad_point, first);
}

} // namespace

// d_in: at least n resident rows, n = 2^log2n, 1 <= log2n <= 22; winv_m261: omega_n^-1, Montgomery-261, canonical 29-bit limbs (host_fr.hpp limbs_m261);
// ninv_plain: n^-1 mod r as a plain integer.  d_find: one SrsCurveFindings the caller has initialised ({0, ~0}); *found is its value after the finish kernel:
// the output rows at infinity.  With none, *d_out_rows is a new allocation of n rows, the caller's, and host_table_out (may be null) the 2n-entry endo table
// of them through the export kernel of bbgpu_srs_generate; with some, *d_out_rows is null and nothing is kept.  ms3 (may be null): the device times of the
// stage kernels, of the load kernel and of the finish kernel, from events between them (bbgpu_set_timing).
int srs_lagrange_rows(const uint32_t* d_in, size_t n, int log2n, const uint32_t winv_m261[9], const uint64_t ninv_plain[4], SrsCurveFindings* d_find,
                      SrsCurveFindings* found, uint32_t** d_out_rows, uint64_t* host_table_out, hipStream_t st, float* ms3)
{
    StageEvents<4> ev;
    *d_out_rows = nullptr;
    if (int rc = ev.create(ms3 != nullptr)) return rc;
    DevBuf scratch, rows;
    HIPCHK(dev_malloc(&scratch.p, n * 128));
    HIPCHK(dev_malloc(&rows.p, n * 64));
    Limbs9 wl;
    for (int i = 0; i < NL; i++) wl.d[i] = winv_m261[i];
    Scalar256 k;
    for (int i = 0; i < 4; i++) k.d[i] = ninv_plain[i];
    const uint32_t n32 = (uint32_t)n, lg = (uint32_t)log2n;
    if (int rc = ev.mark(0, st)) return rc;
    k_lagrange_load<<<(n32 + LT - 1) / LT, LT, 0, st>>>(d_in, scratch.as<uint32_t>(), n32, lg, k);
    if (int rc = ev.mark(1, st)) return rc;
    for (uint32_t s = 0; s < lg; s++) k_lagrange_stage<<<(n32 / 2 + LT - 1) / LT, LT, 0, st>>>(scratch.as<uint32_t>(), n32, lg, s, wl, 0);
    if (int rc = ev.mark(2, st)) return rc;
    k_lagrange_finish<<<(uint32_t)std::min<size_t>((n + FT - 1) / FT, 2048), FT, 0, st>>>(scratch.as<uint32_t>(), rows.as<uint32_t>(), (uint64_t)n, d_find);
    HIPCHK(launch_check()); // the chain: load, stages, finish
    if (int rc = ev.mark(3, st)) return rc;
    HIPCHK(d2h_async(found, d_find, sizeof *found, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ms3) {
        if (int rc = ev.ms(1, 2, &ms3[0])) return rc;
        if (int rc = ev.ms(0, 1, &ms3[1])) return rc;
        if (int rc = ev.ms(2, 3, &ms3[2])) return rc;
    }
    if (found->bad_points) return BBGPU_OK; // no table: the buffers go with this frame
    (void)dev_free(scratch.release<void>());
    if (host_table_out) {
        DevBuf exp;
        HIPCHK(dev_malloc(&exp.p, n * 128));
        if (int rc = srs_export(rows.as<uint32_t>(), n, exp.as<uint32_t>(), st)) return rc;
        if (int rc = device_to_host_sync(host_table_out, exp.p, n * 128, st)) return rc;
    }
    *d_out_rows = rows.release<uint32_t>();
    return BBGPU_OK;
}

} // namespace bbgpu
