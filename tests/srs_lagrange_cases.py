"""Shared cases of the Lagrange-basis SRS tests (tests/test_srs_lagrange_host.py, tests/test_gpu_srs_lagrange.py; test infrastructure, may import oracle/):
the tables and what a conversion must give.  L_i = n^-1 sum_j omega^(-i j) P_j; for the honest table of x that is L_i(x) G with
L_i(x) = (x^n - 1) omega^i / (n (x - omega^i)), computed here in Python integers and multiplied onto the generator by the oracle.  For any table,
sum_i v_i L_i = sum_j ifft(v)_j P_j: the oracle's MSM and transform.  The host and the GPU entry are judged against the same values."""
import numpy as np

from oracle.pyoracle import FQ, FR, FR_MODULUS as R, aligned_copy, from_int, to_int
from tests.srs_update_cases import NONE, all_g_table, honest_table, mont, secret_x, tampered, unrelated_points  # noqa: F401  (re-exported)

ERR_SIZE, ERR_ARG = " -2:", " -3:"


def omega(oracle, n):
    """the root of unity of the size-n domain (the one the transforms use), as a plain integer"""
    return to_int(oracle.from_mont(FR, oracle.root_of_unity(n.bit_length() - 1)))


def lagrange_at(oracle, x, n):
    """[L_i(x)] for a plain integer x outside the domain"""
    w = omega(oracle, n)
    num = (pow(x, n, R) - 1) * pow(n, -1, R) % R
    return [num * pow(w, i, R) * pow((x - pow(w, i, R)) % R, -1, R) % R for i in range(n)]


def generator_times(oracle, scalars):
    """the endo table of [k G] for plain integers k != 0, by the oracle's plain scalar multiplication"""
    g = oracle.g1_one_affine()
    rows = aligned_copy(np.array([oracle.g1_normalize(oracle.g1_scalar_mul(g, mont(oracle, k)))[:8] for k in scalars], dtype=np.uint64))
    return oracle.point_table(rows)


def omega_table(oracle, n, k):
    """the honest table of x = omega^k: L_i(x) = delta_ik, every output row but k is infinity"""
    return honest_table(oracle, mont(oracle, pow(omega(oracle, n), k, R)), n)


def collision_table(oracle, n, j, j2):
    """unrelated rows with row j + n/2 := row j and row j2 + n/2 := -row j2: the first stage doubles at one butterfly and meets an intermediate infinity
    at another; every output row is finite"""
    p = unrelated_points(oracle, n)
    p[j + n // 2] = p[j]
    p[j2 + n // 2, :4] = p[j2, :4]
    p[j2 + n // 2, 4:] = oracle.neg(FQ, p[j2, 4:])
    return oracle.point_table(p)


def identity_holds(oracle, table, lagrange, n, seed):
    """sum_i v_i L_i == sum_j ifft(v)_j P_j for random v"""
    v = oracle.random_scalars(seed, n)
    return np.array_equal(oracle.msm_affine(v, aligned_copy(lagrange), n)[:8], oracle.msm_affine(oracle.ntt(v, "ifft"), aligned_copy(table), n)[:8])


def rows_by_msm(oracle, table, n):
    """every L_i as the oracle's MSM over the n scalars n^-1 omega^(-i j): (n, 8)"""
    w_inv, n_inv = pow(omega(oracle, n), -1, R), pow(n, -1, R)
    out = np.zeros((n, 8), dtype=np.uint64)
    for i in range(n):
        sc = aligned_copy(np.array([mont(oracle, n_inv * pow(w_inv, i * j, R)) for j in range(n)], dtype=np.uint64))
        out[i] = oracle.msm_affine(sc, aligned_copy(table), n)[:8]
    return out
