// kzg_open_all.hip -- the device part of bbgpu_kzg_open_all_setup and bbgpu_kzg_open_all_device (include/bbgpu.h): the KZG proofs pi(omega^i) of a
// polynomial at all n points of its domain, as one structured linear map of the string (Feist and Khovratovich): with N = 2 n, W the N-th root and
//   s = (P_(n-2) .. P_0, infinity x (n + 1)),   t = (c_(n-1), 0 x (n + 1), c_1 .. c_(n-2)),   h = the first n entries of IDFT_N(DFT_N(s) o DFT_N(t)),
// the proofs are the size-n forward transform of (h_0 .. h_(n-2), infinity).  Points live on a scratch of projective points (XYZZ, 128 bytes each, ZZ == 0 for
// infinity; g1_ladder.hpp) and every kernel takes the polynomial of a batch from blockIdx.y:
//   k_open_all_string  (setup) slot i <- s_bitrev(i); log2 N launches of k_lagrange_stage (g1_stage.hpp) with root W leave S^ = DFT_N(s), kept by the handle;
//   k_open_all_t       the batch x N scalars of t from the coefficients; bbgpu_ntt_device_batch transforms them (capi.hip);
//   k_open_all_load    slot i <- (N^-1 t^_bitrev(i)) * S^_bitrev(i): each lane reads its own scalar, brings it to a plain canonical integer by one product
//                      and runs one ladder over a projective base; a zero scalar or an infinite base gives infinity;
//   k_lagrange_stage   log2 N launches with root W^-1: slots [0, n - 1) now hold h;
//   k_open_all_gather  slot n + bitrev_n(m) <- slot m for m < n - 1, slot 2 n - 1 <- infinity: the upper half of a polynomial's slots, dead after the
//                      inverse transform, is the size-n scratch of the forward transform;
//   k_lagrange_stage   log2 n launches with root omega on those upper halves;
//   k_open_all_finish  one Fermat inversion per row to the reference's affine format (Montgomery-256, canonical; infinity: bit 63 of y[3], the rest zero).
// One wave per workgroup, 3-bit windows and no twiddle table, as srs_lagrange.hip.  The reference has no counterpart.
#include <hip/hip_runtime.h>

#include "bbgpu_internal.h"
#include "g1_stage.hpp"

namespace bbgpu {

namespace {

constexpr int FT = 256; // threads per workgroup of the kernels that run no ladder

// slot i of the N <- s_j, j = bitrev(i): row n - 2 - j of the table for j <= n - 2 (ZZ = ZZZ = 1), infinity above
__global__ void __launch_bounds__(FT) k_open_all_string(const uint32_t* __restrict__ in, uint32_t* __restrict__ scratch, uint32_t n, uint32_t log2N)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n) return;
    const uint32_t j = __brev(i) >> (32 - log2N); // log2N >= 2; j < 2 n
    uint32_t o[32];
    if (j <= n - 2) {
        uint32_t w[16];
        const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)(n - 2 - j) * 16); // row < n - 1
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint4 v = src[t];
            w[4 * t] = v.x; w[4 * t + 1] = v.y; w[4 * t + 2] = v.z; w[4 * t + 3] = v.w;
        }
        Pt p;
        ladder_base(p, w);
        store_pt(o, p, false);
    } else {
#pragma unroll
        for (int t = 0; t < 32; t++) o[t] = 0;
    }
    store_words32(scratch + (size_t)i * 32, o);
}

// t_i of polynomial blockIdx.y, i < N = 2 n: c_(n-1) at 0, zero for 1 <= i <= n + 1, c_(i-n-1) above (host_kzg_open_all.hpp kzg_open_all_t_source).  The
// words are copied as they are: the transform takes any representative.
__global__ void __launch_bounds__(FT) k_open_all_t(const uint32_t* __restrict__ coeffs, size_t stride_elems, uint32_t* __restrict__ t, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * n) return;
    const size_t b = blockIdx.y;
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (i == 0 || i > n + 1) {
        const uint32_t src = i == 0 ? n - 1 : i - n - 1; // < n <= stride_elems
        const uint4* c = reinterpret_cast<const uint4*>(coeffs + (b * stride_elems + src) * 8);
        lo = c[0];
        hi = c[1];
    }
    uint4* dst = reinterpret_cast<uint4*>(t + (b * 2 * n + i) * 8);
    dst[0] = lo;
    dst[1] = hi;
}

// slot i of polynomial blockIdx.y <- k * S^_j, j = bitrev(i), k = N^-1 t^_j as a plain canonical integer: t^ is in the memory format (x 2^256, any
// representative), c32 holds the plain integer 32 N^-1 mod r, and the Montgomery-261 product of the two is N^-1 t^_j itself (as k_srs_update brings y^e to an
// integer by a product with the plain one)
__global__ void __launch_bounds__(LT) k_open_all_load(const uint32_t* __restrict__ that, const uint32_t* __restrict__ S, uint32_t* __restrict__ scratch, uint32_t N,
                                                      uint32_t log2N, Limbs9 c32)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const size_t b = blockIdx.y;
    const uint32_t j = __brev(i) >> (32 - log2N); // < N
    uint64_t k[4];
    {
        uint32_t sw[8], kw[8];
        const uint4* src = reinterpret_cast<const uint4*>(that + (b * N + j) * 8);
        const uint4 lo = src[0], hi = src[1];
        sw[0] = lo.x; sw[1] = lo.y; sw[2] = lo.z; sw[3] = lo.w;
        sw[4] = hi.x; sw[5] = hi.y; sw[6] = hi.z; sw[7] = hi.w;
        to_canonical(mul(unpack<FrP>(sw), fe_from<FrP>(c32.d)), kw);
#pragma unroll
        for (int t = 0; t < 4; t++) k[t] = (uint64_t)kw[2 * t] | ((uint64_t)kw[2 * t + 1] << 32);
    }
    uint32_t w[32];
    load_words32(S + (size_t)j * 32, w);
    uint32_t any = 0;
#pragma unroll
    for (int t = 0; t < 8; t++) any |= w[16 + t];
    Pt acc;
    bool inf = true;
    if (any != 0 && (k[0] | k[1] | k[2] | k[3]) != 0) ladder_pt<LAGRANGE_WB>(w, k, acc, inf);
    uint32_t o[32];
    store_pt(o, acc, inf);
    store_words32(scratch + (b * N + i) * 32, o);
}

// the size-n scratch of the forward transform, slots [n, 2 n) of polynomial blockIdx.y: n + bitrev(m) <- slot m for m < n - 1, 2 n - 1 <- infinity
// (bitrev(n - 1) == n - 1).  Reads touch slots below n only and writes slots from n on.
__global__ void __launch_bounds__(FT) k_open_all_gather(uint32_t* __restrict__ scratch, uint32_t n, uint32_t log2n)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    uint32_t* base = scratch + (size_t)blockIdx.y * 2 * n * 32;
    const uint32_t j = __brev(m) >> (32 - log2n); // log2n >= 1; j < n
    uint32_t w[32];
    if (m == n - 1) {
#pragma unroll
        for (int t = 0; t < 32; t++) w[t] = 0;
    } else {
        load_words32(base + (size_t)m * 32, w);
    }
    store_words32(base + (size_t)(n + j) * 32, w);
}

// proof i of polynomial blockIdx.y <- the affine form of slot n + i in the reference's format.  Infinity is an ordinary result: nothing is counted.
__global__ void __launch_bounds__(FT) k_open_all_finish(const uint32_t* __restrict__ scratch, uint32_t* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t b = blockIdx.y;
    uint32_t w[32], o[16];
    load_words32(scratch + (b * 2 * n + n + i) * 32, w);
    Pt p;
    bool inf;
    load_pt(p, inf, w);
    if (inf) {
#pragma unroll
        for (int t = 0; t < 16; t++) o[t] = 0;
        o[15] = 0x80000000u;
    } else {
        const auto inv = fq_inverse_fermat(mul(p.zz, p.zzz));
        const auto izz = mul(inv, p.zzz), izzz = mul(inv, p.zz);
        uint32_t c[8];
        to_canonical(m261_to_m256<Fq>(mul(p.x, izz)), c);
#pragma unroll
        for (int t = 0; t < 8; t++) o[t] = c[t];
        to_canonical(m261_to_m256<Fq>(mul(p.y, izzz)), c);
#pragma unroll
        for (int t = 0; t < 8; t++) o[8 + t] = c[t];
    }
    uint4* dst = reinterpret_cast<uint4*>(out + (b * n + i) * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) dst[t] = make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
}

Limbs9 to_limbs9(const uint32_t v[9])
{
    Limbs9 r;
    for (int i = 0; i < NL; i++) r.d[i] = v[i];
    return r;
}
uint32_t blocks_of(uint32_t count, int threads) { return (count + threads - 1) / threads; }

} // namespace

// d_in: at least n - 1 resident rows on the curve, n = 2^log2n, 1 <= log2n <= 21; W_m261: fr_root_of_unity(log2n + 1), Montgomery-261, canonical 29-bit
// limbs (host_fr.hpp limbs_m261).  *d_S: a new allocation of 2 n scratch points, S^ in natural order, the caller's on success.
int kzg_open_all_string(const uint32_t* d_in, size_t n, int log2n, const uint32_t W_m261[9], uint32_t** d_S, hipStream_t st)
{
    *d_S = nullptr;
    const uint32_t n32 = (uint32_t)n, N = 2 * n32, lgN = (uint32_t)log2n + 1;
    DevBuf S;
    HIPCHK(dev_malloc(&S.p, (size_t)N * 128));
    k_open_all_string<<<blocks_of(N, FT), FT, 0, st>>>(d_in, S.as<uint32_t>(), n32, lgN);
    const Limbs9 W = to_limbs9(W_m261);
    for (uint32_t s = 0; s < lgN; s++) k_lagrange_stage<<<blocks_of(N / 2, LT), LT, 0, st>>>(S.as<uint32_t>(), N, lgN, s, W, 0);
    HIPCHK(launch_check()); // the chain: string, stages
    HIPCHK(hipStreamSynchronize(st));
    *d_S = S.release<uint32_t>();
    return BBGPU_OK;
}

// d_t <- the batch x 2 n scalars of t (d_t: batch x 2 n elements)
int kzg_open_all_t(const uint64_t* d_coeffs, size_t stride_elems, int batch, size_t n, uint64_t* d_t, hipStream_t st)
{
    k_open_all_t<<<dim3(blocks_of((uint32_t)(2 * n), FT), (uint32_t)batch), FT, 0, st>>>((const uint32_t*)d_coeffs, stride_elems, (uint32_t*)d_t, (uint32_t)n);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_that: DFT_N(t) of every polynomial, batch x 2 n elements in the memory format; on return the same buffer holds the batch x n proofs (64 bytes each:
// t^ is dead once the load kernel has run, and is as large).  d_scratch: batch x 2 n scratch points.  c32: the plain integer 32 N^-1 mod r; Winv, omega:
// fr_root_of_unity(log2n + 1)^-1 and fr_root_of_unity(log2n), Montgomery-261 -- all canonical 29-bit limbs.  Nothing is synchronised unless ms4 is given:
// then the device times of the load kernel, the inverse stages, the gather kernel with the forward stages, and the finish kernel (bbgpu_set_timing).
int kzg_open_all_chain(const uint32_t* d_S, uint64_t* d_that, uint32_t* d_scratch, size_t n, int log2n, int batch, const uint32_t c32[9], const uint32_t Winv[9],
                       const uint32_t omega[9], hipStream_t st, float* ms4)
{
    StageEvents<5> ev;
    if (int rc = ev.create(ms4 != nullptr)) return rc;
    const uint32_t n32 = (uint32_t)n, N = 2 * n32, lg = (uint32_t)log2n, lgN = lg + 1, nb = (uint32_t)batch;
    if (int rc = ev.mark(0, st)) return rc;
    k_open_all_load<<<dim3(blocks_of(N, LT), nb), LT, 0, st>>>((const uint32_t*)d_that, d_S, d_scratch, N, lgN, to_limbs9(c32));
    if (int rc = ev.mark(1, st)) return rc;
    const Limbs9 wi = to_limbs9(Winv), om = to_limbs9(omega);
    for (uint32_t s = 0; s < lgN; s++) k_lagrange_stage<<<dim3(blocks_of(N / 2, LT), nb), LT, 0, st>>>(d_scratch, N, lgN, s, wi, (size_t)N);
    if (int rc = ev.mark(2, st)) return rc;
    k_open_all_gather<<<dim3(blocks_of(n32, FT), nb), FT, 0, st>>>(d_scratch, n32, lg);
    for (uint32_t s = 0; s < lg; s++) k_lagrange_stage<<<dim3(blocks_of(n32 / 2, LT), nb), LT, 0, st>>>(d_scratch + (size_t)n32 * 32, n32, lg, s, om, (size_t)N);
    if (int rc = ev.mark(3, st)) return rc;
    k_open_all_finish<<<dim3(blocks_of(n32, FT), nb), FT, 0, st>>>(d_scratch, (uint32_t*)d_that, n32);
    HIPCHK(launch_check()); // the chain: load, stages, gather, stages, finish
    if (ms4) {
        if (int rc = ev.mark(4, st)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < 4; i++)
            if (int rc = ev.ms(i, i + 1, &ms4[i])) return rc;
    }
    return BBGPU_OK;
}

} // namespace bbgpu
