// host_plonk_check.hpp -- does a witness satisfy the circuit?  The definition of include/bbgpu.h (bbgpu_plonk_check_witness) on the host, behind
// bbgpu_host_plonk_check_witness: for a caller without a GPU, and the statement the GPU kernels (poly.hip k_check_gates_lanes / k_check_copies_lanes) are compared with.
// Like host_fallback.hpp: the library's own host field code (host_fr.hpp), a few host threads above 2^15 rows, no HIP call, no lock, no state.
//
// Rows 0 .. n-2 only: the proof system divides by the pseudo vanishing polynomial (polynomial_arithmetic.cpp:478-560) and the grand product stops at
// Z(w^(n-1)) = 1 (prover.cpp:135-222), so row n-1 is constrained neither by its gate nor by its copy constraints.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/bbgpu.h"
#include "host_fr.hpp"

namespace bbgpu {
namespace host {

// any representative below 2^256 < 6r -> canonical
static inline Fr fr_load_any(const uint64_t* v, size_t i)
{
    Fr a;
    memcpy(a.d, v + 4 * i, 32);
    for (int k = 0; k < 5; k++) fr_cond_sub_p(a);
    return a;
}

static inline bbgpu_plonk_witness_report plonk_report_clear()
{
    bbgpu_plonk_witness_report R;
    memset(&R, 0, sizeof R);
    R.first_gate = R.first_copy = R.first_copy_target = BBGPU_PLONK_NONE;
    return R;
}

// rows [i0, i1) of the circuit, i1 <= n - 1
static inline bbgpu_plonk_witness_report plonk_check_rows(const bbgpu_plonk_circuit& c, size_t i0, size_t i1)
{
    bbgpu_plonk_witness_report R = plonk_report_clear();
    const size_t n = c.n, rows = n - 1;
    const uint64_t* wires[3] = { c.w_l, c.w_r, c.w_o };
    const uint32_t* maps[3] = { c.sigma_1_mapping, c.sigma_2_mapping, c.sigma_3_mapping };
    for (size_t i = i0; i < i1; i++) {
        const Fr wl = fr_load_any(c.w_l, i), wr = fr_load_any(c.w_r, i), wo = fr_load_any(c.w_o, i);
        uint32_t k = 0;
        Fr a = fr_mul(fr_mul(fr_load_any(c.q_m, i), wl), wr);
        a = fr_add(a, fr_mul(fr_load_any(c.q_l, i), wl));
        a = fr_add(a, fr_mul(fr_load_any(c.q_r, i), wr));
        a = fr_add(a, fr_mul(fr_load_any(c.q_o, i), wo));
        a = fr_add(a, fr_load_any(c.q_c, i));
        if (c.q_o_next) a = fr_add(a, fr_mul(fr_load_any(c.q_o_next, i), fr_load_any(c.w_o, i + 1)));
        if (!fr_is_zero(a)) k |= BBGPU_PLONK_FAIL_ARITH;
        if (c.q_bl) {
            auto boolean = [&](const uint64_t* q, const Fr& w) { return fr_is_zero(fr_mul(fr_load_any(q, i), fr_sub(fr_sqr(w), w))); };
            if (!boolean(c.q_bl, wl)) k |= BBGPU_PLONK_FAIL_BOOL_L;
            if (!boolean(c.q_br, wr)) k |= BBGPU_PLONK_FAIL_BOOL_R;
            if (!boolean(c.q_bo, wo)) k |= BBGPU_PLONK_FAIL_BOOL_O;
        }
        if (c.q_mimc_selector) {
            const Fr qsel = fr_load_any(c.q_mimc_selector, i);
            const Fr t = fr_add(fr_add(wo, wl), fr_load_any(c.q_mimc_coefficient, i));
            if (!fr_is_zero(fr_mul(qsel, fr_sub(fr_mul(fr_sqr(t), t), wr)))) k |= BBGPU_PLONK_FAIL_MIMC_CUBE;
            if (!fr_is_zero(fr_mul(qsel, fr_sub(fr_mul(t, fr_sqr(wr)), fr_load_any(c.w_o, i + 1))))) k |= BBGPU_PLONK_FAIL_MIMC_OUT;
        }
        if (k) {
            if (R.first_gate == BBGPU_PLONK_NONE) {
                R.first_gate = (uint32_t)i;
                R.first_gate_kinds = k;
            }
            R.kinds |= k;
            R.gate_failures++;
        }
        const Fr own[3] = { wl, wr, wo };
        for (uint32_t wire = 0; wire < 3; wire++) {
            const uint32_t m = maps[wire][i]; // decoded as k_sigma_from_mapping (poly.hip) decodes it
            const size_t row = (m & ((1u << 29) - 1u)) & (n - 1);
            const uint32_t type = (m >> 30) & 3u;
            const uint64_t* src = wires[type == 3 ? 0 : type];
            if (row < rows && fr_eq(fr_load_any(src, row), own[wire])) continue;
            if (R.first_copy == BBGPU_PLONK_NONE) {
                R.first_copy = (uint32_t)i | (wire << 30);
                R.first_copy_target = m;
            }
            R.copy_failures++;
        }
    }
    return R;
}

static inline void plonk_report_append(bbgpu_plonk_witness_report& R, const bbgpu_plonk_witness_report& next) // `next` covers later rows
{
    R.gate_failures += next.gate_failures;
    R.copy_failures += next.copy_failures;
    R.kinds |= next.kinds;
    if (R.first_gate == BBGPU_PLONK_NONE) {
        R.first_gate = next.first_gate;
        R.first_gate_kinds = next.first_gate_kinds;
    }
    if (R.first_copy == BBGPU_PLONK_NONE) {
        R.first_copy = next.first_copy;
        R.first_copy_target = next.first_copy_target;
    }
}

static inline bbgpu_plonk_witness_report plonk_check_witness(const bbgpu_plonk_circuit& c)
{
    const size_t rows = c.n - 1;
    const size_t T = rows < ((size_t)1 << 15) ? 1 : std::min<size_t>(8, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<bbgpu_plonk_witness_report> part(T);
    std::vector<std::thread> pool;
    for (size_t t = 1; t < T; t++) pool.emplace_back([&, t] { part[t] = plonk_check_rows(c, rows * t / T, rows * (t + 1) / T); });
    part[0] = plonk_check_rows(c, 0, rows / T);
    for (std::thread& th : pool) th.join();
    for (size_t t = 1; t < T; t++) plonk_report_append(part[0], part[t]);
    return part[0];
}

} // namespace host
} // namespace bbgpu
