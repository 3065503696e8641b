// fr_mem_device.hpp -- what the KZG check and recovery kernels (kzg_check.hip, kzg_check_cells.hip, kzg_recover_cells.hip, kzg_recover_each.hip) and
// k_g1_verdict of g1_recover.hip share beside the field arithmetic: a field element between memory and registers in two 16-byte accesses, the
// square-and-multiply with a lane-independent trip count, and the workgroup minimum of a pair of findings.  plonk_verify.hip and msm.hip have helpers of
// the same names with other signatures; they include nothing of this.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fe.hpp"

namespace bbgpu {

// the eight 32-bit words of an element, low word first
__device__ __forceinline__ void ld8(const uint64_t* p, uint32_t (&w)[8])
{
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 a = q[0], b = q[1];
    w[0] = (uint32_t)a.x; w[1] = (uint32_t)(a.x >> 32); w[2] = (uint32_t)a.y; w[3] = (uint32_t)(a.y >> 32);
    w[4] = (uint32_t)b.x; w[5] = (uint32_t)(b.x >> 32); w[6] = (uint32_t)b.y; w[7] = (uint32_t)(b.y >> 32);
}
// zero: write the element zero instead (a select per word, so that the lanes of a wave store together either way)
__device__ __forceinline__ void st8(uint64_t* p, const uint32_t (&w)[8], bool zero)
{
    ulonglong2* q = reinterpret_cast<ulonglong2*>(p);
    const uint64_t v0 = w[0] | ((uint64_t)w[1] << 32), v1 = w[2] | ((uint64_t)w[3] << 32), v2 = w[4] | ((uint64_t)w[5] << 32), v3 = w[6] | ((uint64_t)w[7] << 32);
    q[0] = make_ulonglong2(zero ? 0 : v0, zero ? 0 : v1);
    q[1] = make_ulonglong2(zero ? 0 : v2, zero ? 0 : v3);
}
// the four 64-bit words of an element
__device__ __forceinline__ void ld4(const uint64_t* p, uint64_t (&v)[4])
{
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
    const ulonglong2 lo = q[0], hi = q[1];
    v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
}
// base^e over the low `bits` bits of e, most significant first: the same trip count on every lane
__device__ __forceinline__ Fe<FrP, 1, 2> pow_bits(const FeT<FrP>& base, uint32_t e, int bits)
{
    Fe<FrP, 1, 2> acc = fe_one<FrP>();
    for (int b = bits - 1; b >= 0; --b) {
        acc = sqr(acc);
        const Fe<FrP, 1, 2> m = mul(acc, base);
        const bool take = ((e >> b) & 1u) != 0;
#pragma unroll
        for (int i = 0; i < NL; i++) acc.d[i] = take ? m.d[i] : acc.d[i];
    }
    return acc;
}

// The smallest `bad` and the smallest `bug` over a workgroup of THREADS threads, every one of which calls this: __shfl_xor inside a wave, then an LDS
// slot per wave.  True on thread 0 alone, whose bad and bug then hold the two minima; what the other threads hold is of no use.
template <int THREADS>
__device__ __forceinline__ bool min_pair_to_thread0(uint32_t& bad, uint32_t& bug, uint32_t (&s_bad)[THREADS / 64], uint32_t (&s_bug)[THREADS / 64])
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        bad = min(bad, (uint32_t)__shfl_xor((int)bad, o));
        bug = min(bug, (uint32_t)__shfl_xor((int)bug, o));
    }
    if ((threadIdx.x & 63) == 0) {
        s_bad[threadIdx.x >> 6] = bad;
        s_bug[threadIdx.x >> 6] = bug;
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
#pragma unroll
    for (int k = 1; k < THREADS / 64; k++) {
        bad = min(bad, s_bad[k]);
        bug = min(bug, s_bug[k]);
    }
    return true;
}

// ---- for the launchers of those files and of kzg_open_cosets.hip: a kernel argument of nine 29-bit limbs from the host's array, and the grid of a count
static inline Limbs9 to_limbs9(const uint32_t v[9])
{
    Limbs9 r;
    for (int i = 0; i < NL; i++) r.d[i] = v[i];
    return r;
}
static inline uint32_t blocks_of(uint32_t count, int threads) { return (count + threads - 1) / threads; }

} // namespace bbgpu
