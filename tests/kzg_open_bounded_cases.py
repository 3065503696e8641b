"""Shared cases of the bounded open-on-every-coset tests (tests/test_kzg_open_bounded_host.py, tests/test_gpu_kzg_open_bounded.py; test infrastructure, may
import oracle/): a polynomial of degree < d opened on the m = n / l cosets of a domain of size n >= d.  The polynomials are those of
tests/kzg_open_cosets_cases.py at length d (so that every steering case steers the size-mu products, mu = d / l); the reference is the same quotient
definition over the coefficients zero-extended to n.  The bounded construction is restated here over plain integers (bounded_identity_holds), with x^j
standing in for P_j, and held to that definition."""
import numpy as np

from oracle.pyoracle import FR_MODULUS as R, aligned_copy
from tests.kzg_open_cosets_cases import (ERR_ARG, ERR_SIZE, ERR_STATE, INF, PAD, buffer_of, coset_polynomials, honest_table, omega, quotient,  # noqa: F401
                                         reference, secret_x)

IDENTITY_SHAPES = [(16, 2, 8), (32, 4, 8), (32, 1, 16), (32, 4, 32), (64, 4, 16), (16, 4, 8), (32, 2, 4)]  # (n, l, d): mu = 2 and d = n among them


def extended(coeffs, n):
    """(n, 4): the (d, 4) coefficients followed by zeros"""
    out = np.zeros((n, 4), dtype=np.uint64)
    out[:coeffs.shape[0]] = coeffs
    return aligned_copy(out)


def bounded_reference(lib, oracle, table, coeffs, n, l, cosets=None):
    """(len(cosets), 8): pi_k of the degree-< d polynomial `coeffs` ((d, 4)) on the cosets of the size-n domain, by the quotient definition over an n-row
    table"""
    return reference(lib, oracle, table, extended(coeffs, n), l, cosets=cosets)


def bounded_identity_holds(oracle, n, l, d, seed):
    """over plain integers, with P_j := x^j, c of degree < d, m = n / l, mu = d / l, M = 2 mu, psi = omega^l: (i) the first mu entries of
    IDFT_M(sum_e DFT_M(s^(e)) o DFT_M(t^(e))) are (h_0 .. h_(mu-2), 0), h_u = sum_{(u+1) l <= j < d} c_j P_(j - (u+1) l), for
    s^(e) = (P^(e)_(mu-2) .. P^(e)_0, 0 x (mu + 1)) and t^(e) = (c^(e)_(mu-1), 0 x (mu + 1), c^(e)_1 .. c^(e)_(mu-2)); (ii) the forward size-m transform,
    root psi, of (h_0 .. h_(mu-2), 0 x (m - mu + 1)) is q_k(x) at every k < m, q_k by synthetic division of the polynomial on the size-n domain"""
    rng = np.random.default_rng(seed)
    x = int.from_bytes(rng.bytes(32), "little") % R
    c = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(d)]
    m, mu = n // l, d // l
    M = 2 * mu
    psi, W = omega(oracle, m), omega(oracle, M)
    assert mu >= 2 and m % mu == 0 and pow(omega(oracle, n), l, R) == psi
    P = [pow(x, j, R) for j in range(d)]
    ev = lambda q, z: sum(v * pow(z, j, R) for j, v in enumerate(q)) % R  # noqa: E731
    pi = [ev(quotient(c + [0] * (n - d), l, pow(psi, k, R)), x) for k in range(m)]
    h = [sum(c[j] * P[j - (u + 1) * l] for j in range((u + 1) * l, d)) % R for u in range(mu - 1)] + [0]
    dft = lambda v, root: [sum(v[j] * pow(root, j * k, R) for j in range(M)) % R for k in range(M)]  # noqa: E731
    total = [0] * M
    for e in range(l):
        Pe, ce = P[e::l], c[e::l]
        s = [Pe[mu - 2 - i] for i in range(mu - 1)] + [0] * (mu + 1)
        t = [ce[mu - 1]] + [0] * (mu + 1) + ce[1:mu - 1]
        assert len(s) == M and len(t) == M
        total = [(acc + a * b) % R for acc, a, b in zip(total, dft(s, W), dft(t, W))]
    conv = [v * pow(M, -1, R) % R for v in dft(total, pow(W, -1, R))]
    if conv[:mu] != h:
        return False
    padded = h + [0] * (m - mu)
    return [sum(pow(psi, k * u, R) * padded[u] for u in range(m)) % R for k in range(m)] == pi
