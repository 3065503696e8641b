"""Shared cases of the open-on-every-coset tests (tests/test_kzg_open_cosets_host.py, tests/test_gpu_kzg_open_cosets.py; test infrastructure, may import
oracle/): the polynomials and what the m = n / l cell proofs must be.  The reference is the quotient definition, coset by coset: pi_k = the commitment
(bbgpu_host_msm_g1) of q_k, f = q_k (X^l - psi^k) + r_k, with q_k by synthetic division over Python integers -- never the construction under test.  That
construction is restated here over plain integers (cosets_identity_holds), with x^j standing in for P_j, and held to the same definition."""
import numpy as np

from oracle.pyoracle import FR, FR_MODULUS as R, PolyOracle, aligned_copy, to_int
from tests.kzg_open_all_cases import (ERR_ARG, ERR_SIZE, ERR_STATE, INF, PAD, buffer_of, honest_table, infinite_row_table, omega, polynomials,  # noqa: F401
                                      secret_x)

MONT_INV = pow(1 << 256, -1, R)


def plain(coeffs):
    """the plain integers of (n, 4) elements in the memory format, any representative"""
    return [to_int(c) * MONT_INV % R for c in coeffs]


def memory(values):
    return aligned_copy(PolyOracle.mont([v % R for v in values]))


def coset_polynomials(oracle, n, l):
    """[(name, (n, 4) coefficients)]: those of the open-at-every-point cases, and for l >= 2 the ones that steer the sum over residues, x the secret of the
    honest table (S^(e) = x^e S^(0) there, so residue e' with c^(e') = x^(e - e') c^(e) gives the SAME point as residue e at every frequency):
      degree < l           every proof is infinity;
      residue 0 only       c_j = 0 unless l | j: l - 1 of the l products of every frequency are infinity;
      first level doubles  c^(1) = x^-1 c^(0), the other residues random: the tree partners 0 and 1 are equal;
      first level cancels  c^(1) = -x^-1 c^(0): they are opposite, and an infinity travels up the tree;
      last level doubles   c^(e + l/2) = x^(-l/2) c^(e) for every e < l / 2: the two halves of the sum are equal;
      last level cancels   the same with a minus sign: every frequency sums to infinity"""
    out = list(polynomials(oracle, n))
    if l == 1:
        return out
    x = to_int(oracle.from_mont(FR, secret_x(oracle))) % R
    rnd = plain(oracle.random_scalars(0xC05E7 + 64 * n + l, n))
    out.append(("degree < l", memory([v if j < l else 0 for j, v in enumerate(rnd)])))
    out.append(("residue 0 only", memory([v if j % l == 0 else 0 for j, v in enumerate(rnd)])))
    for name, sign in (("first level doubles", 1), ("first level cancels", -1)):
        c, f = list(rnd), sign * pow(x, -1, R)
        for a in range(n // l):
            c[1 + l * a] = f * c[l * a]
        out.append((name, memory(c)))
    for name, sign in (("last level doubles", 1), ("last level cancels", -1)):
        c, f = list(rnd), sign * pow(x, -(l // 2), R)
        for j in range(n):
            if j % l >= l // 2:
                c[j] = f * c[j - l // 2]
        out.append((name, memory(c)))
    return out


def quotient(c, l, z):
    """q with f = q (X^l - z) + r, deg r < l, over plain integers: q_d = c_(d+l) + z q_(d+l); n entries, the top l zero"""
    n = len(c)
    q = [0] * n
    for d in range(n - l - 1, -1, -1):
        q[d] = (c[d + l] + z * (q[d + l] if d + l < n else 0)) % R
    return q


def reference(lib, oracle, table, coeffs, l, cosets=None):
    """(len(cosets), 8): pi_k for the cosets k asked for (all m by default) by the quotient definition -- synthetic division, then bbgpu_host_msm_g1
    over the same table rows"""
    n = coeffs.shape[0]
    m = n // l
    c, t, psi = plain(coeffs), aligned_copy(table[:2 * n]), omega(oracle, m)
    cosets = range(m) if cosets is None else cosets
    return np.array([lib.host_msm(memory(quotient(c, l, pow(psi, k, R))), t, n)[:8] for k in cosets], dtype=np.uint64)


def fold_single_proofs(lib, oracle, singles, n, l):
    """(m, 8): pi_k = sum_j [omega^(k + m j) / (l psi^k)] pi(omega^(k + m j)) from the (n, 8) finite single proofs, an l-point bbgpu_host_msm_g1 per cell"""
    m, w = n // l, omega(oracle, n)
    out = np.zeros((m, 8), dtype=np.uint64)
    for k in range(m):
        inv = pow(l * pow(w, l * k, R), -1, R)
        sc = memory([pow(w, k + m * j, R) * inv for j in range(l)])
        out[k] = lib.host_msm(sc, oracle.point_table(aligned_copy(singles[k::m])), l)[:8]
    return out


def cosets_identity_holds(oracle, n, l, seed):
    """over plain integers, with P_j := x^j, m = n / l, M = 2 m, psi = omega^l: (i) the forward size-m transform, root psi, of (h_0 .. h_(m-2), 0),
    h_u = sum_{j >= (u+1) l} c_j P_(j - (u+1) l), is q_k(x) at every k; (ii) the first m entries of IDFT_M(sum_e DFT_M(s^(e)) o DFT_M(t^(e))) are h, for
    s^(e) = (P^(e)_(m-2) .. P^(e)_0, 0 x (m + 1)) and t^(e) = (c^(e)_(m-1), 0 x (m + 1), c^(e)_1 .. c^(e)_(m-2)); (iii) pi_k is the partial-fraction
    fold of the single proofs on its coset"""
    rng = np.random.default_rng(seed)
    x = int.from_bytes(rng.bytes(32), "little") % R
    c = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]
    m = n // l
    M = 2 * m
    w, psi, W = omega(oracle, n), omega(oracle, m), omega(oracle, M)
    assert m >= 2 and pow(w, l, R) == psi
    P = [pow(x, j, R) for j in range(n)]
    ev = lambda q, z: sum(v * pow(z, j, R) for j, v in enumerate(q)) % R  # noqa: E731
    pi = [ev(quotient(c, l, pow(psi, k, R)), x) for k in range(m)]
    h = [sum(c[j] * P[j - (u + 1) * l] for j in range((u + 1) * l, n)) % R for u in range(m - 1)] + [0]
    if [sum(pow(psi, k * u, R) * h[u] for u in range(m)) % R for k in range(m)] != pi:
        return False
    dft = lambda v, root: [sum(v[j] * pow(root, j * k, R) for j in range(M)) % R for k in range(M)]  # noqa: E731
    total = [0] * M
    for e in range(l):
        Pe, ce = P[e::l], c[e::l]
        s = [Pe[m - 2 - i] for i in range(m - 1)] + [0] * (m + 1)
        t = [ce[m - 1]] + [0] * (m + 1) + ce[1:m - 1]
        assert len(s) == M and len(t) == M
        total = [(acc + a * b) % R for acc, a, b in zip(total, dft(s, W), dft(t, W))]
    conv = [v * pow(M, -1, R) % R for v in dft(total, pow(W, -1, R))]
    if conv[:m] != h:
        return False
    single = lambda z: (ev(c, x) - ev(c, z)) * pow((x - z) % R, -1, R) % R  # noqa: E731
    for k in range(m):
        zs = [pow(w, k + m * j, R) for j in range(l)]
        if sum(z * pow(l * pow(psi, k, R), -1, R) * single(z) for z in zs) % R != pi[k]:
            return False
    return True
