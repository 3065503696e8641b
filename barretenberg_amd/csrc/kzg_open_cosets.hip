// kzg_open_cosets.hip -- the device part of bbgpu_kzg_open_cosets_setup and bbgpu_kzg_open_cosets_device, and of bbgpu_kzg_open_all_setup and
// bbgpu_kzg_open_all_device, which are the coset size l = 1 without a bound (include/bbgpu.h): the KZG proof pi_k of a polynomial on every coset
// { omega^(k + m j) : j < l } of its domain, m = n / l cosets of l points, by the multi-proof construction of Feist and Khovratovich
// (host_kzg_open_cosets.hpp states it).  At l = 1 that is one structured linear map of the string: with N = 2 n, W the N-th root and
//   s = (P_(n-2) .. P_0, infinity x (n + 1)),   t = (c_(n-1), 0 x (n + 1), c_1 .. c_(n-2)),   h = the first n entries of IDFT_N(DFT_N(s) o DFT_N(t)),
// the proofs are the size-n forward transform of (h_0 .. h_(n-2), infinity).  For l > 1 string and coefficients are split by residue e = j mod l into l
// problems of that layout at size m, whose products are SUMMED in the Fourier domain: with M = 2 m and W the M-th root, one inverse transform of length M and one forward transform of length m
// serve all l residues.  Points live on a scratch of projective points (XYZZ, 128 bytes each, ZZ == 0 for infinity; g1_ladder.hpp) and every per-call kernel
// takes the polynomial of a batch from blockIdx.y.  A setup carries a degree bound d, 2 l <= d <= n (bbgpu_kzg_open_cosets_setup_bounded; d = n without one):
// the Toeplitz products then have size mu = d / l, M = 2 mu, and only the last forward transform lives on the size-m domain, rho = m / mu:
//   k_open_cosets_string (setup) slot i of transform e <- s^(e)_bitrev(i); log2 M launches of k_lagrange_stage (g1_stage.hpp), gridDim.y = l, with root W
//                        leave S^(e) = DFT_M(s^(e)), l x M = 2 d points kept by the handle;
//   k_open_cosets_t      the batch x l x M scalars of t^(e) from the coefficients; bbgpu_ntt_device_batch transforms them (capi.hip);
//   k_open_cosets_sum    slot i <- sum_e (M^-1 t^^(e)_j) * S^(e)_j, j = bitrev(i): lane (f, e) of a wave runs the ladder of residue e at the wave's f-th
//                        frequency, then the l results of a frequency are added in a log2 l-level tree across lanes, through LDS (no level at l = 1: every
//                        lane stores its own product);
//   k_lagrange_stage     log2 M launches with root W^-1: slots [0, mu - 1) now hold h;
//   k_open_cosets_gather slot m + rho bitrev_mu(u) + c <- slot u for u < mu - 1 and every c < rho, the rho slots of u = mu - 1 <- infinity: the size-m
//                        input (h_0 .. h_(mu-2), infinity x (m - mu + 1)) in bit-reversed order is nonzero at multiples of rho only, and stages 0 ..
//                        log2 rho - 1 of the decimation in time would turn every (a, infinity) into (a, a) -- the gather writes those copies itself;
//   k_lagrange_stage     stages log2 rho .. log2 m - 1 of the size-m transform with root omega^l on those upper halves (all log2 m at d = n);
//   k_open_cosets_finish one Fermat inversion per row to the reference's affine format (affine_from_scratch, g1_ladder.hpp).
// Every polynomial owns 2 m scratch slots whatever d is: the convolution in [0, M), M <= 2 m, the forward transform in [m, 2 m) (M <= m when d < n, and at
// d = n the gather reads below m and writes from m on).  At d = n every launch, index and result is that of the construction without a bound.  One wave per
// workgroup, 3-bit windows and no twiddle table, as srs_lagrange.hip.  The reference has no counterpart.
#include <hip/hip_runtime.h>

#include "bbgpu_internal.h"
#include "fr_mem_device.hpp"
#include "g1_stage.hpp"

namespace bbgpu {

namespace {

constexpr int FT = 256; // threads per workgroup of the kernels that run no ladder

// slot i of transform e, g = e M + i < l M = 2 d <- s^(e)_j, j = bitrev_M(i): row e + l (mu - 2 - j) of the table for j <= mu - 2 (ZZ = ZZZ = 1), infinity
// above.  m here is mu = d / l.
__global__ void __launch_bounds__(FT) k_open_cosets_string(const uint32_t* __restrict__ in, uint32_t* __restrict__ scratch, uint32_t m, uint32_t log2M, uint32_t log2l)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (2 * m) << log2l) return;
    const uint32_t e = g >> log2M, i = g & (2 * m - 1);
    const uint32_t j = __brev(i) >> (32 - log2M); // log2M >= 2; j < 2 m
    uint32_t o[32];
    if (j <= m - 2) {
        uint32_t w[16];
        const uint4* src = reinterpret_cast<const uint4*>(in + (size_t)(e + ((m - 2 - j) << log2l)) * 16); // row <= l - 1 + l (mu - 2) < d - l
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
    store_words32(scratch + (size_t)g * 32, o);
}

// t^(e)_i of polynomial blockIdx.y, g = e M + i < 2 d, m here mu = d / l: c_(e + l (mu - 1)) at i == 0, zero for 1 <= i <= mu + 1, c_(e + l (i - mu - 1))
// above (host_kzg_open_cosets.hpp kzg_open_cosets_t_source).  The words are copied as they are: the transform takes any representative.  Coefficients from
// d on are not read.
__global__ void __launch_bounds__(FT) k_open_cosets_t(const uint32_t* __restrict__ coeffs, size_t stride_elems, uint32_t* __restrict__ t, uint32_t m, uint32_t log2M,
                                                      uint32_t log2l)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x, n2 = (2 * m) << log2l;
    if (g >= n2) return;
    const size_t b = blockIdx.y;
    const uint32_t e = g >> log2M, i = g & (2 * m - 1);
    uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
    if (i == 0 || i > m + 1) {
        const uint32_t src = e + ((i == 0 ? m - 1 : i - m - 1) << log2l); // <= l - 1 + l (mu - 1) < d <= stride_elems
        const uint4* c = reinterpret_cast<const uint4*>(coeffs + (b * stride_elems + src) * 8);
        lo = c[0];
        hi = c[1];
    }
    uint4* dst = reinterpret_cast<uint4*>(t + (b * n2 + g) * 8);
    dst[0] = lo;
    dst[1] = hi;
}

// slot i of polynomial blockIdx.y <- sum_{e < l} k_e * S^(e)_j, j = bitrev_M(i), k_e = M^-1 t^^(e)_j as a plain canonical integer (t^^ is in the memory
// format, x 2^256, any representative, c32 holds the plain integer 32 M^-1 mod r, and the Montgomery-261 product of the two is M^-1 t^^ itself, as
// k_srs_update brings y^e to an integer by a product with the plain one).  Thread g = i l + e: the l lanes of a frequency are neighbours, a wave takes 64 / l
// frequencies.  Each lane runs its own ladder (a zero scalar or an infinite base gives infinity; so does a lane past the end, which arises for l M < 64
// only), then level d of the tree adds the point of lane e + 2^d to that of every lane e with e mod 2^(d+1) == 0.  The points cross in LDS as 32 canonical
// words, word w of lane L at w * 64 + L (consecutive lanes on consecutive banks).  The addition is complete: either side may be infinity, equal points
// double and opposite ones give infinity (add_pt), as two residues of an honest string meet whenever their scalars are in the string's own ratio.  The
// slots of polynomial b start at b * slots (2 m of the domain, >= M).
__global__ void __launch_bounds__(LT) k_open_cosets_sum(const uint32_t* __restrict__ that, const uint32_t* __restrict__ S, uint32_t* __restrict__ scratch, uint32_t M,
                                                        uint32_t log2M, uint32_t log2l, Limbs9 c32, size_t slots)
{
    __shared__ uint32_t cross[32 * LT];
    const uint32_t lane = threadIdx.x, g = blockIdx.x * LT + lane; // < 2^22 + 64
    const uint32_t e = g & ((1u << log2l) - 1u), i = g >> log2l;
    const size_t b = blockIdx.y;
    Pt acc;
    bool inf = true;
    if (i < M) {
        const uint32_t j = __brev(i) >> (32 - log2M); // < M
        uint64_t k[4];
        {
            uint32_t sw[8], kw[8];
            const uint4* src = reinterpret_cast<const uint4*>(that + ((((b << log2l) + e) << log2M) + j) * 8);
            const uint4 lo = src[0], hi = src[1];
            sw[0] = lo.x; sw[1] = lo.y; sw[2] = lo.z; sw[3] = lo.w;
            sw[4] = hi.x; sw[5] = hi.y; sw[6] = hi.z; sw[7] = hi.w;
            to_canonical(mul(unpack<FrP>(sw), fe_from<FrP>(c32.d)), kw);
#pragma unroll
            for (int t = 0; t < 4; t++) k[t] = (uint64_t)kw[2 * t] | ((uint64_t)kw[2 * t + 1] << 32);
        }
        uint32_t w[32];
        load_words32(S + (((size_t)e << log2M) + j) * 32, w);
        uint32_t any = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) any |= w[16 + t];
        if (any != 0 && (k[0] | k[1] | k[2] | k[3]) != 0) ladder_pt<LAGRANGE_WB>(w, k, acc, inf);
    }
#pragma unroll 1
    for (uint32_t bit = 1; bit >> log2l == 0; bit <<= 1) { // wave-uniform: every lane meets every barrier
        const uint32_t r = e & (2 * bit - 1);
        if (r == bit) {
            uint32_t o[32];
            store_pt(o, acc, inf);
#pragma unroll
            for (int t = 0; t < 32; t++) cross[t * LT + lane] = o[t];
        }
        __syncthreads();
        if (r == 0) {
            uint32_t o[32];
#pragma unroll
            for (int t = 0; t < 32; t++) o[t] = cross[t * LT + (lane ^ bit)]; // e + bit < l: the same frequency, the same wave
            Pt p;
            bool pinf;
            load_pt(p, pinf, o);
            if (!pinf) {
                Operand q;
                q.x = p.x;
                q.zz = p.zz;
                q.zzz = p.zzz;
#pragma unroll
                for (int t = 0; t < NL; t++) q.y.d[t] = p.y.d[t];
                add_pt(acc, inf, q);
            }
        }
        __syncthreads(); // the next level writes the words this one read
    }
    if (e == 0 && i < M) {
        uint32_t o[32];
        store_pt(o, acc, inf);
        store_words32(scratch + (b * slots + i) * 32, o);
    }
}

// the size-m scratch of the forward transform, slots [m, 2 m) of polynomial blockIdx.y, after its first log2 rho stages, rho = m / mu: thread q = u rho + c
// copies slot u < mu - 1 (h_u) to slot m + rho bitrev_mu(u) + c, and the rho threads of u = mu - 1 write infinity (bitrev(mu - 1) == mu - 1).  Reads touch
// slots below mu <= m only and writes slots from m on.  At rho = 1 thread u writes slot m + bitrev_m(u).
__global__ void __launch_bounds__(FT) k_open_cosets_gather(uint32_t* __restrict__ scratch, uint32_t m, uint32_t log2mu, uint32_t log2rho)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    uint32_t* base = scratch + (size_t)blockIdx.y * 2 * m * 32;
    const uint32_t u = q >> log2rho, c = q & ((1u << log2rho) - 1u); // u < mu
    const uint32_t j = __brev(u) >> (32 - log2mu);                    // log2mu >= 1; j < mu
    uint32_t w[32];
    if (u == (1u << log2mu) - 1u) {
#pragma unroll
        for (int t = 0; t < 32; t++) w[t] = 0;
    } else {
        load_words32(base + (size_t)u * 32, w);
    }
    store_words32(base + (size_t)(m + (j << log2rho) + c) * 32, w); // < 2 m
}

// proof k of polynomial blockIdx.y <- the affine form of slot m + k in the reference's format.  Infinity is an ordinary result: nothing is counted.
__global__ void __launch_bounds__(FT) k_open_cosets_finish(const uint32_t* __restrict__ scratch, uint32_t* __restrict__ out, uint32_t m)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const size_t b = blockIdx.y;
    uint32_t w[32], o[16];
    load_words32(scratch + (b * 2 * m + m + i) * 32, w);
    affine_from_scratch(w, o);
    uint4* dst = reinterpret_cast<uint4*>(out + (b * m + i) * 16);
#pragma unroll
    for (int t = 0; t < 4; t++) dst[t] = make_uint4(o[4 * t], o[4 * t + 1], o[4 * t + 2], o[4 * t + 3]);
}

} // namespace

// d_in: at least d - l resident rows on the curve, d = 2^log2d, l = 2^log2l, 0 <= log2l <= 6, 1 <= log2d - log2l, log2d <= 21; W_m261:
// fr_root_of_unity(log2d - log2l + 1), Montgomery-261, canonical 29-bit limbs (host_fr.hpp limbs_m261).  *d_S: a new allocation of 2 d scratch points,
// S^(e) in natural order at e M, the caller's on success.
int kzg_open_cosets_string(const uint32_t* d_in, int log2d, int log2l, const uint32_t W_m261[9], uint32_t** d_S, hipStream_t st)
{
    *d_S = nullptr;
    const uint32_t lgl = (uint32_t)log2l, lgM = (uint32_t)(log2d - log2l) + 1, M = 1u << lgM, l = 1u << lgl;
    DevBuf S;
    HIPCHK(dev_malloc(&S.p, ((size_t)M << lgl) * 128));
    k_open_cosets_string<<<blocks_of(M << lgl, FT), FT, 0, st>>>(d_in, S.as<uint32_t>(), M / 2, lgM, lgl);
    const Limbs9 W = to_limbs9(W_m261);
    for (uint32_t s = 0; s < lgM; s++) k_lagrange_stage<<<dim3(blocks_of(M / 2, LT), l), LT, 0, st>>>(S.as<uint32_t>(), M, lgM, s, W, (size_t)M);
    HIPCHK(launch_check()); // the chain: string, stages
    HIPCHK(hipStreamSynchronize(st));
    *d_S = S.release<uint32_t>();
    return BBGPU_OK;
}

// d_t <- the batch x l x M scalars of t^(e), M = 2 d / l, transform e of polynomial b at (b l + e) M (d_t: batch x 2 d elements)
int kzg_open_cosets_t(const uint64_t* d_coeffs, size_t stride_elems, int batch, int log2d, int log2l, uint64_t* d_t, hipStream_t st)
{
    const uint32_t lgM = (uint32_t)(log2d - log2l) + 1;
    k_open_cosets_t<<<dim3(blocks_of(2u << log2d, FT), (uint32_t)batch), FT, 0, st>>>((const uint32_t*)d_coeffs, stride_elems, (uint32_t*)d_t, 1u << (lgM - 1), lgM,
                                                                                      (uint32_t)log2l);
    HIPCHK(launch_check());
    return BBGPU_OK;
}

// d_that: DFT_M(t^(e)) of every polynomial and residue, batch x 2 d elements in the memory format, in a buffer that also takes the batch x m proofs (64 bytes
// each), which it holds on return.  d_scratch: batch x 2 m scratch points.  c32: the plain integer 32 M^-1 mod r; Winv, psi: fr_root_of_unity(log2 M)^-1 and
// fr_root_of_unity(log2 m), Montgomery-261 -- all canonical 29-bit limbs.  Nothing is synchronised unless ms4 is given: then the device times of the sum
// kernel, the inverse stages, the gather kernel with the forward stages, and the finish kernel (bbgpu_set_timing).
int kzg_open_cosets_chain(const uint32_t* d_S, uint64_t* d_that, uint32_t* d_scratch, int log2n, int log2l, int log2d, int batch, const uint32_t c32[9],
                          const uint32_t Winv[9], const uint32_t psi[9], hipStream_t st, float* ms4)
{
    StageEvents<5> ev;
    if (int rc = ev.create(ms4 != nullptr)) return rc;
    const uint32_t lgl = (uint32_t)log2l, lgm = (uint32_t)(log2n - log2l), lgmu = (uint32_t)(log2d - log2l), lgM = lgmu + 1, lgrho = lgm - lgmu;
    const uint32_t m = 1u << lgm, M = 2u << lgmu, nb = (uint32_t)batch;
    const size_t slots = 2 * (size_t)m; // per polynomial
    if (int rc = ev.mark(0, st)) return rc;
    k_open_cosets_sum<<<dim3(blocks_of(M << lgl, LT), nb), LT, 0, st>>>((const uint32_t*)d_that, d_S, d_scratch, M, lgM, lgl, to_limbs9(c32), slots);
    if (int rc = ev.mark(1, st)) return rc;
    const Limbs9 wi = to_limbs9(Winv), ps = to_limbs9(psi);
    for (uint32_t s = 0; s < lgM; s++) k_lagrange_stage<<<dim3(blocks_of(M / 2, LT), nb), LT, 0, st>>>(d_scratch, M, lgM, s, wi, slots);
    if (int rc = ev.mark(2, st)) return rc;
    k_open_cosets_gather<<<dim3(blocks_of(m, FT), nb), FT, 0, st>>>(d_scratch, m, lgmu, lgrho);
    for (uint32_t s = lgrho; s < lgm; s++) k_lagrange_stage<<<dim3(blocks_of(m / 2, LT), nb), LT, 0, st>>>(d_scratch + (size_t)m * 32, m, lgm, s, ps, slots);
    if (int rc = ev.mark(3, st)) return rc;
    k_open_cosets_finish<<<dim3(blocks_of(m, FT), nb), FT, 0, st>>>(d_scratch, (uint32_t*)d_that, m);
    HIPCHK(launch_check()); // the chain: sum, stages, gather, stages, finish
    if (ms4) {
        if (int rc = ev.mark(4, st)) return rc;
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < 4; i++)
            if (int rc = ev.ms(i, i + 1, &ms4[i])) return rc;
    }
    return BBGPU_OK;
}

} // namespace bbgpu
