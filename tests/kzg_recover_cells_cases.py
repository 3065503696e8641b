"""Shared cases of the recover-from-cells tests (tests/test_kzg_recover_cells_host.py, tests/test_gpu_kzg_recover_cells.py; test infrastructure, may
import oracle/): seeded polynomials of degree < d, their cells by a transform over Python integers, the sets of missing cells, and an INDEPENDENT recovery
-- Lagrange interpolation over Python integers through the listed points, which never forms the vanishing polynomial the library works with.  The ground
truth of a recovery is the polynomial one started from; for altered data it is the interpolation (the unique polynomial of degree < count l through the
listed values, which is what the library's D is)."""
import functools

import numpy as np

from oracle.pyoracle import FR_MODULUS as R, PolyOracle, aligned_copy, from_int, to_int

ERR_HIP, ERR_SIZE, ERR_ARG = " -1:", " -2:", " -3:"
PAD = 5
MONT_INV = pow(1 << 256, -1, R)
ALL_ONES = (1 << 256) - 1  # a representative the library reduces: the value (2^256 - 1) / 2^256


def log2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def omega(n):
    return PolyOracle.root(log2(n))


def memory(values):
    """(len, 4): canonical, in the memory format"""
    return aligned_copy(PolyOracle.mont([v % R for v in values]))


def plain(words):
    """the plain integers of (k, 4) elements in the memory format, any representative"""
    return [to_int(w) * MONT_INV % R for w in np.asarray(words).reshape(-1, 4)]


def transform(c, n):
    """[f(omega^i) for i < n] of the coefficients c (at most n), over Python integers: radix 2, decimation in time"""
    a = list(c) + [0] * (n - len(c))
    lg = log2(n)
    for i in range(n):
        j = int(format(i, "0%db" % lg)[::-1], 2) if lg else 0
        if i < j:
            a[i], a[j] = a[j], a[i]
    size = 2
    while size <= n:
        w, half = omega(size), size // 2
        tw = [1] * half
        for j in range(1, half):
            tw[j] = tw[j - 1] * w % R
        for k in range(0, n, size):
            for j in range(half):
                u, v = a[k + j], a[k + j + half] * tw[j] % R
                a[k + j], a[k + j + half] = (u + v) % R, (u - v) % R
        size *= 2
    return a


@functools.lru_cache(maxsize=None)
def polynomial(n, d, b=0):
    """(coefficients, values): polynomial b of degree EXACTLY d - 1 on the size-n domain, seeded; tuples of Python integers"""
    rng = np.random.default_rng([0x2EC0, n, d, b])
    c = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(d)]
    c[-1] = c[-1] or 1
    return tuple(c + [0] * (n - d)), tuple(transform(c, n))


def listed_values(values, n, l, cells):
    """(len(cells) * l) integers: point j of listed cell t is f(omega^(cell[t] + m j))"""
    m = n // l
    return [values[k + m * j] for k in cells for j in range(l)]


def call_values(polys, n, l, cells):
    """the `values` argument of one call, (batch * count * l, 4), from the value tuples of the polynomials"""
    return memory([v for vals in polys for v in listed_values(vals, n, l, cells)])


def coefficient_buffer(batch, stride, seed=0xF111):
    """(batch * stride, 4) of other values: what a call's output lies in, so that untouched elements show"""
    rng = np.random.default_rng(seed)
    return aligned_copy(rng.integers(0, 1 << 63, size=(batch * stride, 4), dtype=np.uint64))


def missing_sets(n, l, d, seed=1):
    """{name: sorted missing cells}: every kind of set that fits count l >= d.  none; exactly one; the maximum m - ceil(d / l); the first cells; the last
    cells; every even cell (Z = Y^(m/2) - 1 in Y = X^l); a seeded random set"""
    m = n // l
    most = m - (d + l - 1) // l
    rng = np.random.default_rng([0x5E75, n, l, d, seed])
    out = {"none": []}
    if most >= 1:
        some = min(most, max(1, m // 3))
        out["one"] = [int(rng.integers(m))]
        out["most"] = sorted(int(k) for k in rng.permutation(m)[:most])
        out["first"] = list(range(some))
        out["last"] = list(range(m - some, m))
        out["random"] = sorted(int(k) for k in rng.permutation(m)[:int(rng.integers(1, most + 1))])
    if m // 2 <= most:
        out["even"] = list(range(0, m, 2))
    return out


def present_cells(n, l, missing, seed=2):
    """the cells that are not missing, in a seeded shuffled order, as uint32"""
    gone = set(missing)
    cells = [k for k in range(n // l) if k not in gone]
    np.random.default_rng([0x0DE2, n, l, len(missing), seed]).shuffle(cells)
    return np.array(cells, dtype=np.uint32)


def interpolate(n, l, cells, vals):
    """the n coefficients of the unique polynomial of degree < len(cells) * l with value vals[t * l + j] at omega^(cells[t] + m j): Lagrange's formula over
    Python integers, O(N^2) -- for n <= 64"""
    assert n <= 64
    m, w = n // l, omega(n)
    xs = [pow(w, int(k) + m * j, R) for k in cells for j in range(l)]
    N = len(xs)
    master = [1]  # prod (X - x_i), lowest coefficient first
    for x in xs:
        master = [((master[i - 1] if i else 0) - x * (master[i] if i < len(master) else 0)) % R for i in range(len(master) + 1)]
    out = [0] * n
    for x, y in zip(xs, vals):
        q, carry = [0] * N, 0  # master / (X - x) by synthetic division from the top
        for i in range(N, 0, -1):
            carry = (master[i] + x * carry) % R
            q[i - 1] = carry
        den = 0
        for cq in reversed(q):
            den = (den * x + cq) % R
        f = y * pow(den, -1, R) % R
        for i in range(N):
            out[i] = (out[i] + f * q[i]) % R
    return out


def expected_report(coeffs_by_poly, d, present, mu):
    """the report the definition gives for the recovered coefficient lists"""
    rep = dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, missing=mu)
    for b, c in enumerate(coeffs_by_poly):
        bad = [i for i in range(d, present) if c[i] % R]
        if bad:
            return dict(consistent=0, first_bad_poly=b, first_bad_coeff=bad[0], missing=mu)
    return rep


def add_modulus(words, rows):
    """the same elements with r added to the rows given: another representative below 2^256"""
    out = words.copy()
    for i in rows:
        out[i] = from_int(to_int(out[i]) + R)
    return out
