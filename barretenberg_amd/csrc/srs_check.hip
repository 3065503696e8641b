// srs_check.hip -- the two O(n) device parts of bbgpu_srs_check (include/bbgpu.h) that are not an MSM: the curve test over the resident rows and the
// random multipliers.  The sums A and B are the existing device MSM (two tickets over one scalar vector, capi.hip); the pairing is host code
// (host_pairing.hpp).  The reference tests curve membership with g1::on_curve per point on the CPU (test/test_io.cpp:12-34) and has no batched form.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bbgpu_internal.h"
#include "g1.hpp"

namespace bbgpu {

#define HIPCHK(x)                                                                                                      \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) {                                                                                        \
            set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));                                \
            return BBGPU_ERR_HIP;                                                                                      \
        }                                                                                                              \
    } while (0)

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
// The device twin of keccak.hpp's permutation (FIPS 202: theta, rho, pi, chi, iota), written for registers: the 25 lanes are indexed by compile-time
// constants only (every loop over the state is unrolled), the round constants come from constant memory by the uniform round number.  The message is
// 40 bytes, one block of the rate (136): lanes 0-3 the seed, lane 4 the index, the padding byte 0x01 opens lane 5 and 0x80 closes lane 16.
__constant__ uint64_t KECCAK_RC[24] = { 0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
                                        0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
                                        0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
                                        0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
                                        0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL };

template <int S> __device__ __forceinline__ uint64_t rotl64c(uint64_t x)
{
    if constexpr (S == 0) return x;
    else return (x << S) | (x >> (64 - S));
}
// B[y + 5 ((2x + 3y) mod 5)] = rotl(A[x + 5y], rotation offset of lane (x, y)), for one lane
template <int X, int Y> __device__ __forceinline__ void rho_pi_lane(const uint64_t (&A)[25], uint64_t (&B)[25])
{
    constexpr int ROT[25] = { 0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14 }; // index x + 5y
    B[Y + 5 * ((2 * X + 3 * Y) % 5)] = rotl64c<ROT[X + 5 * Y]>(A[X + 5 * Y]);
}
template <int Y> __device__ __forceinline__ void rho_pi_row(const uint64_t (&A)[25], uint64_t (&B)[25])
{
    rho_pi_lane<0, Y>(A, B);
    rho_pi_lane<1, Y>(A, B);
    rho_pi_lane<2, Y>(A, B);
    rho_pi_lane<3, Y>(A, B);
    rho_pi_lane<4, Y>(A, B);
}
__device__ __forceinline__ void keccak_f1600_device(uint64_t (&A)[25])
{
#pragma unroll 1
    for (int round = 0; round < 24; round++) {
        uint64_t C[5], D[5], B[25];
#pragma unroll
        for (int x = 0; x < 5; x++) C[x] = A[x] ^ A[x + 5] ^ A[x + 10] ^ A[x + 15] ^ A[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) D[x] = C[(x + 4) % 5] ^ rotl64c<1>(C[(x + 1) % 5]);
#pragma unroll
        for (int i = 0; i < 25; i++) A[i] ^= D[i % 5];
        rho_pi_row<0>(A, B);
        rho_pi_row<1>(A, B);
        rho_pi_row<2>(A, B);
        rho_pi_row<3>(A, B);
        rho_pi_row<4>(A, B);
#pragma unroll
        for (int y = 0; y < 5; y++)
#pragma unroll
            for (int x = 0; x < 5; x++) A[x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y]);
        A[0] ^= KECCAK_RC[round];
    }
}

struct Seed {
    uint64_t d[4];
};
__global__ void __launch_bounds__(CT) k_srs_check_scalars(Seed seed, uint64_t count, uint64_t* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    uint64_t A[25];
#pragma unroll
    for (int k = 0; k < 25; k++) A[k] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) A[k] = seed.d[k];
    A[4] = i;
    A[5] = 0x01;
    A[16] = 0x8000000000000000ULL;
    keccak_f1600_device(A);
    ulonglong2* o = reinterpret_cast<ulonglong2*>(out + 4 * i);
    o[0] = make_ulonglong2(A[0], A[1]);
    o[1] = make_ulonglong2(A[2], A[3] & 0x1FFFFFFFFFFFFFFFULL);
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
