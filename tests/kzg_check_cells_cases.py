"""Shared cases of the tests of the check of KZG cell proofs (tests/test_kzg_check_cells_host.py, tests/test_gpu_kzg_check_cells.py; test infrastructure,
may import oracle/).  Worlds come from tests/kzg_open_cosets_cases.py: the honest table of a known secret, polynomials, the host proofs
(bbgpu_host_kzg_open_cosets, held to the quotient definition by tests/test_kzg_open_cosets_host.py); the values are bbgpu_host_ntt's.  The independent
reference: r_k by naive Lagrange interpolation over Python integers (never an inverse transform), the multipliers by a Keccak-256 written out here, A and
B by bbgpu_host_msm_g1 over scalars made in Python, the verdict cell by cell with bbgpu_host_pairing_check.  Nothing here calls the entries under test."""
import numpy as np

from oracle.pyoracle import FR, FR_MODULUS as R, aligned_copy, to_int
from tests.kzg_check_cases import (ERR_ARG, ERR_SIZE, NONE, SCALARS, SEED, above_r, honest, negated, off_curve, plus_one, scalars)  # noqa: F401
from tests.kzg_open_cosets_cases import INF, honest_table, memory, omega, plain, secret_x
from tests.srs_check_cases import g2_of
from tests.srs_update_cases import mont

SIZES = [(2, 1), (4, 2), (8, 4), (16, 8), (32, 16), (64, 32), (128, 64)]  # every l at the smallest n with m >= 2
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R)

# ---- Keccak-256 (the original padding 0x01, not SHA-3's) ----
_RC = [0x0000000000000001, 0x0000000000008082, 0x800000000000808A, 0x8000000080008000, 0x000000000000808B, 0x0000000080000001, 0x8000000080008081,
       0x8000000000008009, 0x000000000000008A, 0x0000000000000088, 0x0000000080008009, 0x000000008000000A, 0x000000008000808B, 0x800000000000008B,
       0x8000000000008089, 0x8000000000008003, 0x8000000000008002, 0x8000000000000080, 0x000000000000800A, 0x800000008000000A, 0x8000000080008081,
       0x8000000000008080, 0x0000000080000001, 0x8000000080008008]
_ROT = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]
_M64 = (1 << 64) - 1


def _rol(v, s):
    return ((v << s) | (v >> (64 - s))) & _M64 if s else v


def _keccak_f(A):
    for rc in _RC:
        Cc = [A[x][0] ^ A[x][1] ^ A[x][2] ^ A[x][3] ^ A[x][4] for x in range(5)]
        D = [Cc[(x - 1) % 5] ^ _rol(Cc[(x + 1) % 5], 1) for x in range(5)]
        A = [[A[x][y] ^ D[x] for y in range(5)] for x in range(5)]
        B = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                B[y][(2 * x + 3 * y) % 5] = _rol(A[x][y], _ROT[x][y])
        A = [[B[x][y] ^ (~B[(x + 1) % 5][y] & _M64 & B[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        A[0][0] ^= rc
    return A


def keccak256(msg):
    rate = 136
    assert len(msg) < rate
    block = bytearray(msg) + bytearray(rate - len(msg))
    block[len(msg)] ^= 0x01
    block[rate - 1] ^= 0x80
    A = [[0] * 5 for _ in range(5)]
    for i in range(rate // 8):
        A[i % 5][i // 5] ^= int.from_bytes(block[8 * i:8 * i + 8], "little")
    A = _keccak_f(A)
    return b"".join(A[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


assert keccak256(b"").hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"


def rho(seed, t):
    """the multiplier of item t as an integer: Keccak-256(seed || t) read little-endian, the top three bits cleared"""
    msg = b"".join(int(v).to_bytes(8, "little") for v in seed) + int(t).to_bytes(8, "little")
    return int.from_bytes(keccak256(msg), "little") & ((1 << 253) - 1)


# ---- worlds ----
def power_of_secret(oracle, e):
    """x^e in the memory format, x the secret of the honest table"""
    x = to_int(oracle.from_mont(FR, secret_x(oracle))) % R
    return mont(oracle, pow(x, e, R))


def make_world(lib, oracle, tmp_path, n, l, batch, coeffs=None):
    """`batch` polynomials of n coefficients over the honest string, their cell proofs for cosets of l points: table (2n, 8), head (l, 8), g2_x, g2_xl,
    g2 (the generator), coeffs (batch, n, 4), commitments (batch, 8), values (batch, n, 4) -- the size-n transforms --, proofs (batch, n / l, 8)"""
    x = secret_x(oracle)
    table = honest_table(oracle, x, n)
    if coeffs is None:
        coeffs = oracle.random_scalars(0xCE11 + 131 * n + 7 * l + batch, batch * n)
    coeffs = aligned_copy(np.asarray(coeffs, dtype=np.uint64).reshape(batch, n, 4))
    commitments = np.stack([lib.host_msm(aligned_copy(coeffs[b]), table, n)[:8] for b in range(batch)])
    proofs = lib.host_kzg_open_cosets(table, n, l, aligned_copy(coeffs.reshape(-1, 4)), batch=batch)
    values = np.stack([lib.host_ntt(aligned_copy(coeffs[b]), "fft") for b in range(batch)])
    return dict(n=n, l=l, m=n // l, batch=batch, table=table, head=aligned_copy(table[0:2 * l:2]), g2_x=g2_of(lib, oracle, tmp_path, x, "x.dat"),
                g2_xl=g2_of(lib, oracle, tmp_path, power_of_secret(oracle, l), "xl.dat"), g2=g2_of(lib, oracle, tmp_path, oracle.const(FR, "one"), "one.dat"),
                coeffs=coeffs, commitments=commitments, values=values, proofs=proofs)


def cells_of(W, count, start=0):
    """`count` true cells in the labelled form, the polynomials mixed and the cells in scrambled order, with duplicates once count exceeds batch x m:
    (which, cell, values (count * l, 4), proofs (count, 8))"""
    t = np.arange(start, start + count)
    b, k = t % W["batch"], (t * 7 + t // W["batch"]) % W["m"]
    values = np.stack([W["values"][bb, kk::W["m"]] for bb, kk in zip(b, k)]).reshape(-1, 4)
    return b.astype(np.uint32), k.astype(np.uint32), aligned_copy(values), aligned_copy(W["proofs"][b, k])


def args_of(W, which, cell, values, proofs, commitments=None, g2_xl=None, head=None):
    """the positional arguments of kzg_check_cells / host_kzg_check_cells"""
    return (W["commitments"] if commitments is None else commitments, which, cell, values, proofs, W["n"], W["l"], W["head"] if head is None else head,
            W["g2_xl"] if g2_xl is None else g2_xl)


def cosets_args(W, values=None, proofs=None, commitments=None, g2_xl=None):
    """the positional arguments of kzg_check_open_cosets / host_kzg_check_open_cosets (values unpadded unless given)"""
    return (W["commitments"] if commitments is None else commitments, aligned_copy(W["values"].reshape(-1, 4)) if values is None else values,
            W["proofs"] if proofs is None else proofs, W["n"], W["l"], W["head"], W["g2_xl"] if g2_xl is None else g2_xl)


def padded(oracle, W, pad):
    """the transforms at stride n + pad, other values between them"""
    n, stride = W["n"], W["n"] + pad
    buf = aligned_copy(oracle.random_scalars(0x57D + n, W["batch"] * stride))
    for b in range(W["batch"]):
        buf[b * stride:b * stride + n] = W["values"][b]
    return buf, stride


# ---- the independent reference ----
def interpolate(zs, vs):
    """the coefficients of the polynomial of degree < len(zs) through (zs[j], vs[j]): naive Lagrange over plain integers"""
    l = len(zs)
    out = [0] * l
    for j in range(l):
        num, den = [1], 1  # prod_{i != j} (X - z_i), prod_{i != j} (z_j - z_i)
        for i in range(l):
            if i != j:
                num = [(a - zs[i] * b) % R for a, b in zip([0] + num, num + [0])]
                den = den * (zs[j] - zs[i]) % R
        f = vs[j] * pow(den, -1, R) % R
        out = [(o + f * c) % R for o, c in zip(out, num)]
    return out


def msm(lib, oracle, scalars, points):
    """sum scalars[i] points[i] over plain integers and affine points, infinities left out: (8,)"""
    keep = [i for i, p in enumerate(points) if not (int(p[7]) >> 63) & 1]
    if not keep:
        return INF.copy()
    pts = aligned_copy(np.stack([points[i] for i in keep]))
    return lib.host_msm(memory([scalars[i] for i in keep]), oracle.point_table(pts), len(keep))[:8]


def pairing_holds(lib, oracle, W, a, b, g2_xl):
    """e(a, G2) e(-b, g2_xl) == 1, a pair whose point is at infinity left out"""
    ps, qs = [], []
    if not (int(a[7]) >> 63) & 1:
        ps.append(a)
        qs.append(W["g2"])
    if not (int(b[7]) >> 63) & 1:
        ps.append(negated(oracle, b))
        qs.append(g2_xl)
    return True if not ps else lib.host_pairing_check(np.stack(ps), np.stack(qs))


def reference(lib, oracle, W, commitments, which, cell, values, proofs, head, g2_xl, seed=SEED):
    """dict(a, b, ok, first_failing): A and B of the definition with the EFFECTIVE multipliers rho_t 2^-256 (the sums read scalars in the memory format,
    the multipliers are handed over as they stand), the verdict of the batch, and the first cell whose own check e(C - r_k(x) G + psi^k pi, G2) =
    e(pi, [x^l] G2) fails (-1: none)"""
    n, l, m = W["n"], W["l"], W["m"]
    w = omega(oracle, n)
    psi = pow(w, l, R)
    vals = plain(np.asarray(values).reshape(-1, 4))
    head_rows = [head[i] for i in range(l)]
    sc_c, sc_h, sc_p, sc_b = [0] * len(commitments), [0] * l, [], []
    first_failing = -1
    for t in range(len(which)):
        k = int(cell[t])
        r_k = interpolate([pow(w, k + m * j, R) for j in range(l)], vals[t * l:(t + 1) * l])
        rt = rho(seed, t) * MONT_INV % R
        sc_c[int(which[t])] += rt
        for i in range(l):
            sc_h[i] -= rt * r_k[i]
        sc_p.append(rt * pow(psi, k, R) % R)
        sc_b.append(rt)
        if first_failing < 0:
            own = msm(lib, oracle, [1] + [-c % R for c in r_k] + [pow(psi, k, R)], [commitments[int(which[t])]] + head_rows + [proofs[t]])
            if not pairing_holds(lib, oracle, W, own, proofs[t], g2_xl):
                first_failing = t
    a = msm(lib, oracle, [s % R for s in sc_c + sc_h] + sc_p, list(commitments) + head_rows + list(proofs))
    b = msm(lib, oracle, sc_b, list(proofs))
    return dict(a=[int(v) for v in a], b=[int(v) for v in b], ok=1 if pairing_holds(lib, oracle, W, a, b, g2_xl) else 0, first_failing=first_failing)


def cosets_as_labelled(W, values=None, proofs=None):
    """the cells of the open-cosets form written out in the labelled form: cell t = b m + k"""
    m, l, n, batch = W["m"], W["l"], W["n"], W["batch"]
    v = W["values"] if values is None else np.asarray(values).reshape(batch, n, 4)
    p = W["proofs"] if proofs is None else np.asarray(proofs).reshape(batch, m, 8)
    t = np.arange(batch * m)
    vals = np.stack([v[bb, kk::m] for bb, kk in zip(t // m, t % m)]).reshape(-1, 4)
    return (t // m).astype(np.uint32), (t % m).astype(np.uint32), aligned_copy(vals), aligned_copy(p.reshape(-1, 8))
