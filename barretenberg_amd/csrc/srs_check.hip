// srs_check.hip -- the two O(n) device parts of bbgpu_srs_check (include/bbgpu.h) that are not an MSM: the curve test over the resident rows and the
// random multipliers.  The sums A and B are the existing device MSM (two tickets over one scalar vector, capi.hip); the pairing is host code
// (host_pairing.hpp).  The reference tests curve membership with g1::on_curve per point on the CPU (test/test_io.cpp:12-34) and has no batched form.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "g1.hpp"
#include "keccak_device.hpp"

namespace bbgpu {

namespace {

constexpr int CT = 256; // threads per workgroup, both kernels

struct RowWords {
    uint32_t w[16];
};

// ---- curve test: one thread per resident row (Montgomery-261, canonical, 64 bytes: what the MSM kernels read), strided -----------------------------
// y^2 - x^3 - 3 with the lazy field type: y y + (K p - x^2) x in one shared reduction, minus 3 R, and ONE more product (by R mod p, i.e. by one) whose
// result has exact limbs and a value below 2p -- zero modulo p iff it is 0 or p (is_zero_mulout, as k_check_gates_lanes tests its identities).
// Findings meet on chip -- shuffles inside a wave, an LDS slot per wave -- and ONE thread per workgroup issues the count atomicAdd and the first-row
// atomicMin, only if the workgroup found anything: an honest table issues no atomic, and sums and minima do not depend on arrival order.
// Row 0 is compared with the generator's resident form by the thread that holds it (a plain vector store of the verdict).
__global__ void __launch_bounds__(CT) k_srs_on_curve(const uint32_t* __restrict__ srs, uint64_t n, RowWords generator, SrsCurveFindings* __restrict__ out)
{
    __shared__ unsigned long long s_first[CT / 64];
    __shared__ uint32_t s_bad[CT / 64];
    const uint64_t nt = (uint64_t)gridDim.x * blockDim.x;
    const FeT<Fq> one = fe_one<Fq>();
    const auto three = add(add(one, one), one);
    uint32_t bad = 0;
    unsigned long long first = ~0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += nt) {
        uint32_t w[16];
        const uint4* q = reinterpret_cast<const uint4*>(srs + i * 16);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 v = q[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
        AffineV<1> a;
        load_affine_m261(a, w);
        const auto d = mul_sub(a.y, a.y, sqr(a.x), a.x); // (y^2 - x^3) R
        if (!is_zero_mulout(mul(sub(d, three), one))) {
            bad++;
            first = i < first ? i : first;
        }
        if (i == 0) {
            uint32_t diff = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) diff |= w[k] ^ generator.w[k];
            out->first_is_generator = diff == 0 ? 1u : 0u;
        }
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
    atomicAdd(&out->bad_points, (unsigned long long)bad);
    atomicMin(&out->first_bad_point, first);
}

// ---- multipliers: rho_i = Keccak-256(seed || i) with the top three bits cleared, one thread per scalar ------------------------------------------------
// The permutation and the one-block message are keccak_device.hpp's (shared with plonk_verify.hip).
__global__ void __launch_bounds__(CT) k_srs_check_scalars(Seed seed, uint64_t count, uint64_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t r[4];
    keccak_rho_device(seed, i, r);
    ulonglong2* o = reinterpret_cast<ulonglong2*>(out + 4 * i);
    o[0] = make_ulonglong2(r[0], r[1]);
    o[1] = make_ulonglong2(r[2], r[3]);
}

} // namespace

// d_out: one SrsCurveFindings the caller has initialised ({0, ~0, 0}); generator_m261: the generator (1, 2) in the resident form, 8 words
int srs_check_curve(const uint32_t* d_srs, size_t n, const uint64_t generator_m261[8], SrsCurveFindings* d_out, hipStream_t st)
{
    RowWords g;
    for (int k = 0; k < 8; k++) {
        g.w[2 * k] = (uint32_t)generator_m261[k];
        g.w[2 * k + 1] = (uint32_t)(generator_m261[k] >> 32);
    }
    const uint32_t blocks = (uint32_t)std::min<size_t>((n + CT - 1) / CT, 2048); // the rest by the stride
    k_srs_on_curve<<<blocks, CT, 0, st>>>(d_srs, (uint64_t)n, g, d_out);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_out: count x 4 words
int srs_check_scalars(const uint64_t seed[4], size_t count, uint64_t* d_out, hipStream_t st)
{
    if (count == 0) return BBGPU_OK;
    Seed s;
    for (int k = 0; k < 4; k++) s.d[k] = seed[k];
    k_srs_check_scalars<<<(uint32_t)((count + CT - 1) / CT), CT, 0, st>>>(s, (uint64_t)count, d_out);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

} // namespace bbgpu
