// host_kzg_check.hpp -- the check of KZG openings (include/bbgpu.h, bbgpu_host_kzg_check_openings): k claims "the polynomial committed to by C_t takes
// the value y_t at z_t, and pi_t is the commitment of its quotient" hold when
//   e(sum_t rho_t (C_t - y_t G + z_t pi_t), G2) e(-sum_t rho_t pi_t, x G2) == 1
// for multipliers rho_t unknown to whoever made the proofs: each claim alone is e(C - y G + z pi, G2) = e(pi, x G2), i.e. C - y G = (x - z) pi, and a
// random combination of false claims holds with probability ~2^-253.  The multipliers, the seed rule, the verdict on x G2 and the verdict on a point are
// host_random_check.hpp's; the sums and the pairing are the batch check's over a call with one commitment per claim (host_kzg_check_batch.hpp,
// kzg_check_host), which takes 2^20 claims where this entry keeps its limit of 64.  Product code, no oracle/; no HIP call, no lock.
#pragma once
#include <stddef.h>

#include "host_random_check.hpp"

namespace bbgpu {
namespace host {

constexpr size_t KZG_CHECK_MAX_OPENINGS = 64;

} // namespace host
} // namespace bbgpu
