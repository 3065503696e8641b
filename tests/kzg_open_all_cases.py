"""Shared cases of the open-at-every-point tests (tests/test_kzg_open_all_host.py, tests/test_gpu_kzg_open_all.py; test infrastructure, may import
oracle/): the polynomials, the strings, and what the n proofs must be.  The reference is the quotient definition, point by point, through entries the
library had before: pi(omega^i) = the commitment (bbgpu_host_msm_g1) of the coefficients of (f(X) - f(omega^i)) / (X - omega^i)
(bbgpu_host_kate_opening) -- never the Toeplitz construction under test.  That construction is restated here over plain integers
(toeplitz_identity_holds), with x^j standing in for P_j, and held to the same definition."""
import numpy as np

from oracle.pyoracle import FR_MODULUS as R, PolyOracle, aligned_copy, from_int
from tests.srs_lagrange_cases import omega
from tests.srs_update_cases import honest_table, lam, mont, secret_x  # noqa: F401  (re-exported)

ERR_SIZE, ERR_ARG, ERR_STATE = " -2:", " -3:", " -4:"
INF = np.array([0, 0, 0, 0, 0, 0, 0, 1 << 63], dtype=np.uint64)
PAD = 5


def polynomials(oracle, n):
    """[(name, (n, 4) coefficients in the memory format)]: random; all zero; constant (every proof is infinity); X (every proof is the generator);
    c X^(n-1) (h_m = c P_(n-2-m)); X + X^(n-1) for n >= 4 (t^_k = 0 at k = n/2 and 3n/2: the load meets zero scalars); coefficients given as r + small;
    coefficients given as 2^256 - 1"""
    rnd = oracle.random_scalars(0x0A11 + n, n)
    one = PolyOracle.mont([1])[0]

    def sparse(entries):
        c = np.zeros((n, 4), dtype=np.uint64)
        for j, v in entries:
            c[j] = v
        return aligned_copy(c)
    out = [("random", aligned_copy(rnd)), ("zero", sparse([])), ("constant", sparse([(0, rnd[0])])), ("X", sparse([(1, one)])),
           ("c X^(n-1)", sparse([(n - 1, rnd[1])]))]
    if n >= 4:
        out.append(("X + X^(n-1)", sparse([(1, one), (n - 1, one)])))
    out.append(("r + small", aligned_copy(np.array([from_int(R + 3 * j + (j == 2)) for j in range(n)], dtype=np.uint64))))
    out.append(("2^256 - 1", aligned_copy(np.array([from_int((1 << 256) - 1)] * n, dtype=np.uint64))))
    return out


def buffer_of(oracle, polys, stride):
    """the (len(polys) * stride, 4) input of one call: polynomial b at row b * stride, the rows between the polynomials filled with other values"""
    n = polys[0].shape[0]
    buf = aligned_copy(oracle.random_scalars(0xBADF + stride, len(polys) * stride))
    for b, c in enumerate(polys):
        buf[b * stride:b * stride + n] = c
    return buf


def domain(oracle, n):
    """omega^i, i < n, in the memory format: (n, 4)"""
    w = omega(oracle, n)
    return aligned_copy(PolyOracle.mont([pow(w, i, R) for i in range(n)]))


def reference(lib, oracle, table, coeffs):
    """(n, 8): the proof at every omega^i by the quotient definition -- bbgpu_host_kate_opening, then bbgpu_host_msm_g1 over the same rows"""
    n = coeffs.shape[0]
    c, t = aligned_copy(coeffs), aligned_copy(table[:2 * n])
    out = np.zeros((n, 8), dtype=np.uint64)
    for i, z in enumerate(domain(oracle, n)):
        q, _ = lib.host_kate_opening(c, z)
        out[i] = lib.host_msm(aligned_copy(q), t, n)[:8]
    return out


def infinite_row_table(oracle, n=4):
    """the honest table of x = W zeta, W the 2n-th root and zeta a primitive cube root of unity in Fr: at n = 4, (W^k / x)^(n-1) = 1 for k = 1 while
    W^k != x, so row 1 of S^ = DFT_2n(s) is the point at infinity"""
    x = omega(oracle, 2 * n) * lam(oracle) % R
    assert n == 4 and pow(lam(oracle), 3, R) == 1 and lam(oracle) != 1
    s_hat_1 = sum(pow(omega(oracle, 2 * n), i, R) * pow(x, n - 2 - i, R) for i in range(n - 1)) % R
    assert s_hat_1 == 0
    return honest_table(oracle, mont(oracle, x), n)


def toeplitz_identity_holds(oracle, n, seed):
    """over plain integers, with P_j := x^j: (i) the forward size-n transform of (h_0 .. h_(n-2), 0), h_m = sum_{j>m} c_j P_(j-m-1), is the quotient
    commitment (f(x) - f(w^i)) / (x - w^i) at every i; (ii) the first n entries of IDFT_N(DFT_N(s) o DFT_N(t)) are h, for
    s = (P_(n-2) .. P_0, 0 x (n + 1)) and t = (c_(n-1), 0 x (n + 1), c_1 .. c_(n-2))"""
    rng = np.random.default_rng(seed)
    x = int.from_bytes(rng.bytes(32), "little") % R
    c = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    w, W, N = omega(oracle, n), omega(oracle, 2 * n), 2 * n
    P = [pow(x, j, R) for j in range(n)]
    h = [sum(c[j] * P[j - m - 1] for j in range(m + 1, n)) % R for m in range(n - 1)] + [0]
    f = lambda z: sum(c[j] * pow(z, j, R) for j in range(n)) % R  # noqa: E731
    for i in range(n):
        z = pow(w, i, R)
        direct = (f(x) - f(z)) * pow((x - z) % R, -1, R) % R
        if sum(pow(z, m, R) * h[m] for m in range(n)) % R != direct:
            return False
    s = [P[n - 2 - i] for i in range(n - 1)] + [0] * (n + 1)
    t = [c[n - 1]] + [0] * (n + 1) + c[1:n - 1]
    assert len(s) == N and len(t) == N
    dft = lambda v, root: [sum(v[j] * pow(root, j * k, R) for j in range(N)) % R for k in range(N)]  # noqa: E731
    prod = [a * b % R for a, b in zip(dft(s, W), dft(t, W))]
    conv = [v * pow(N, -1, R) % R for v in dft(prod, pow(W, -1, R))]
    return conv[:n] == h
