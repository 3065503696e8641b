// keccak_device.hpp -- the device twin of keccak.hpp's permutation (FIPS 202: theta, rho, pi, chi, iota), written for registers: the 25 lanes are
// indexed by compile-time constants only (every loop over the state is unrolled), the round constants come from constant memory by the uniform round
// number.  Shared by the multipliers of bbgpu_srs_check (srs_check.hip) and the transcripts and multipliers of bbgpu_plonk_verify_batch
// (plonk_verify.hip); every translation unit that includes it carries its own copy of the round constants (no relocatable device code).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bbgpu {

static __constant__ uint64_t KECCAK_RC[24] = { 0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
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

// rho_i = Keccak-256(seed || i) with the top three bits cleared (host_srs_check.hpp srs_check_rho): the message is 40 bytes, one block of the rate
// (136): lanes 0-3 the seed, lane 4 the index, the padding byte 0x01 opens lane 5 and 0x80 closes lane 16
struct Seed {
    uint64_t d[4];
};
__device__ __forceinline__ void keccak_rho_device(const Seed& seed, uint64_t i, uint64_t (&out)[4])
{
    uint64_t A[25];
#pragma unroll
    for (int k = 0; k < 25; k++) A[k] = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) A[k] = seed.d[k];
    A[4] = i;
    A[5] = 0x01;
    A[16] = 0x8000000000000000ULL;
    keccak_f1600_device(A);
    out[0] = A[0];
    out[1] = A[1];
    out[2] = A[2];
    out[3] = A[3] & 0x1FFFFFFFFFFFFFFFULL;
}

} // namespace bbgpu
