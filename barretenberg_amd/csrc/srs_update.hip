// srs_update.hip -- the device part of bbgpu_srs_update (include/bbgpu.h): row i of a resident table becomes y^(first_power + i) * P_i, one lane per row.
// The reference has no such operation (its strings come from a file, io.hpp:159-181); what it has is the pieces: the endomorphism split of a scalar
// (fields/field.hpp:413-485, restated for the host in host_wnaf.hpp) and fixed windows of odd signed digits (groups/wnaf.hpp:15-55).  Here both run per
// lane: k = y^e as a plain integer, k = k1 - lambda k2 with |k1|, |k2| < 2^128, then ONE ladder over both halves -- k P = k1 P + k2 (beta x, -y), since
// (beta x, -y) = -lambda P under Fq::BETA and the lambda of host_wnaf.hpp (checked against the oracle, tests/test_srs_update_host.py) -- so 126 shared
// doublings instead of 254.  The split, the group law and the ladder live in g1_ladder.hpp (shared with srs_lagrange.hip); the curve test, the G2 half and
// the registration of the new table are capi.hip's.
#include <hip/hip_runtime.h>

#include "bbgpu_internal.h"
#include "g1_ladder.hpp"

namespace bbgpu {

namespace {

using Fr = FrP;
constexpr int UT = 64; // threads per workgroup: one wave, as srs_gen_points_kernel (250 VGPRs: two waves per SIMD whatever the workgroup)

BB_HD void endo_split_words(const uint64_t* k_in, uint64_t* out6)
{
    const uint64_t k[4] = { k_in[0], k_in[1], k_in[2], k_in[3] };
    EndoSplit s;
    endo_split(k, s);
    out6[0] = s.k1[0];
    out6[1] = s.k1[1];
    out6[2] = s.k2[0];
    out6[3] = s.k2[1];
    out6[4] = (s.neg1 ? 1u : 0u) | (s.neg2 ? 2u : 0u) | (s.fits ? 0u : 4u);
    out6[5] = 0;
}
__global__ void __launch_bounds__(UT) k_selftest_endo_split(const uint64_t* __restrict__ k, uint64_t n, uint64_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    endo_split_words(k + 4 * i, out + 6 * i);
}

// out[i] = y^(first_power + i) * in[i]; in and out may not overlap
template <int WB>
__global__ void __launch_bounds__(UT) k_srs_update(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n, uint64_t first_power, Limbs9 y261)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // s = y^(first_power + i) in Fr (Montgomery-261), then the plain canonical integer -- as srs_gen_points_kernel
    uint64_t k[4];
    {
        Fe<Fr, 1, 2> s = fe_one<Fr>(), b = fe_from<Fr>(y261.d);
        for (uint64_t e = first_power + i; e; e >>= 1) {
            if (e & 1) s = mul(s, b);
            b = sqr(b);
        }
        FeT<Fr> one_raw = fe_zero<Fr>();
        one_raw.d[0] = 1;
        uint32_t kw[8];
        to_canonical(mul(s, one_raw), kw);
#pragma unroll
        for (int t = 0; t < 4; t++) k[t] = (uint64_t)kw[2 * t] | ((uint64_t)kw[2 * t + 1] << 32);
    }
    uint32_t w[16], o[16];
    const uint4* src = reinterpret_cast<const uint4*>(in + i * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint4 v = src[t];
        w[4 * t] = v.x; w[4 * t + 1] = v.y; w[4 * t + 2] = v.z; w[4 * t + 3] = v.w;
    }
    ladder_row<WB>(w, k, o);
    uint4* dst = reinterpret_cast<uint4*>(out + i * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) dst[t] = make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
}

// 3-bit windows: four table entries, 250 VGPRs, no scratch, two waves per SIMD: 16.4 ms per 2^20 rows.  2-bit windows (two entries, 178 VGPRs, still two
// waves) pay 42 more additions per row: 19.9 ms; 4-bit windows (eight entries) need 256 VGPRs and 140 AGPRs of spills and leave one wave per SIMD: 17.7 ms
// (profiles/srs_update.txt).
constexpr int SRS_UPDATE_WB = 3;

} // namespace

// d_in: n resident rows; *d_out_rows: a new allocation of n rows, the caller's on success; host_table_out (may be null): the 2n-entry endo table of the new
// rows, through the export kernel of bbgpu_srs_generate.  y_mont256: Montgomery 2^256, any representative.  first_power + n <= 2^32 (the caller checks).
// kernel_ms (may be null): the device time of k_srs_update alone, from a pair of events around it (bbgpu_set_timing).
int srs_update_rows(const uint32_t* d_in, size_t n, uint64_t first_power, const uint64_t* y_mont256, uint32_t** d_out_rows, uint64_t* host_table_out, hipStream_t st,
                    float* kernel_ms)
{
    StageEvents<2> ev;
    if (int rc = ev.create(kernel_ms != nullptr)) return rc;
    DevBuf rows;
    HIPCHK(dev_malloc(&rows.p, n * 64));
    // y: Montgomery 2^256 -> 2^261, canonical limbs
    uint32_t w[8];
    for (int i = 0; i < 4; i++) { w[2 * i] = (uint32_t)y_mont256[i]; w[2 * i + 1] = (uint32_t)(y_mont256[i] >> 32); }
    Fe<Fr, 1, 2> y261 = m256_to_m261<Fr>(unpack<Fr>(w));
    uint32_t cw[8];
    to_canonical(y261, cw);
    Fe<Fr, 1, 6> yc = unpack<Fr>(cw);
    Limbs9 yl;
    for (int i = 0; i < NL; i++) yl.d[i] = yc.d[i];
    const uint32_t blocks = (uint32_t)((n + UT - 1) / UT); // n <= 2^32: at most 2^26 workgroups
    if (int rc = ev.mark(0, st)) return rc;
    k_srs_update<SRS_UPDATE_WB><<<blocks, UT, 0, st>>>(d_in, rows.as<uint32_t>(), (uint64_t)n, first_power, yl);
    HIPCHK(launch_check());
    if (int rc = ev.mark(1, st)) return rc;
    if (host_table_out) {
        DevBuf exp;
        HIPCHK(dev_malloc(&exp.p, n * 128));
        if (int rc = srs_export(rows.as<uint32_t>(), n, exp.as<uint32_t>(), st)) return rc;
        if (int rc = device_to_host_sync(host_table_out, exp.p, n * 128, st)) return rc;
    }
    HIPCHK(hipStreamSynchronize(st));
    if (kernel_ms)
        if (int rc = ev.ms(0, 1, kernel_ms)) return rc;
    *d_out_rows = rows.release<uint32_t>();
    return BBGPU_OK;
}

} // namespace bbgpu

using namespace bbgpu;

#pragma GCC visibility push(default)
extern "C" {

int bbgpu_selftest_endo_split(int on_device, const uint64_t* k, size_t n, uint64_t* out)
{
    if (!k || !out || n == 0 || n > (1u << 20)) return BBGPU_ERR_ARG;
    if (!on_device) {
        for (size_t i = 0; i < n; i++) endo_split_words(k + 4 * i, out + 6 * i);
        return BBGPU_OK;
    }
    if (bbgpu_device_count() == 0) {
        set_error("no HIP device available: libbbgpu has no CPU fallback");
        return BBGPU_ERR_HIP;
    }
    uint64_t *dk = nullptr, *dout = nullptr;
    int rc = BBGPU_ERR_HIP;
    do {
        if (hipMalloc((void**)&dk, n * 32) != hipSuccess || hipMalloc((void**)&dout, n * 48) != hipSuccess) break;
        if (hipMemcpy(dk, k, n * 32, hipMemcpyHostToDevice) != hipSuccess) break;
        k_selftest_endo_split<<<(uint32_t)((n + UT - 1) / UT), UT>>>(dk, (uint64_t)n, dout);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out, dout, n * 48, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = BBGPU_OK;
    } while (0);
    if (rc) set_error("selftest: HIP failure (%s)", hipGetErrorString(hipGetLastError()));
    if (dk) (void)hipFree(dk);
    if (dout) (void)hipFree(dout);
    return rc;
}

} // extern "C"
#pragma GCC visibility pop
