"""MSM inputs whose points COLLIDE, with a reference that involves no bucket method (test infrastructure; imports oracle/).

Tables are P_i = x^i G for an x of small multiplicative order, so that the table holds few distinct points:
  x = 1: every point is G;  x = -1: G, -G, G, ...;  a 4th / 8th root of unity: 4 / 8 points, each next to its negative (x^(k/2) = -1);
  x = 2: G, 2G, 4G, ... -- all distinct, but related by powers of two, which is what makes rows of DIFFERENT windows of a window
  table (row (w, i) = 2^off[w] P_i) equal.
For such a table the MSM is (sum s_i x^i mod r) G: one big-integer sum and one scalar multiplication.

All scalars here are handled as the RAW integers of their Montgomery limbs (what the MSM entries take): the scalar a limb vector m names is
m / 2^256 mod r, the sum is linear, so sum m_i x^i mod r is again the raw form of the result's scalar -- exactly what oracle.g1_scalar_mul takes.
"""
import numpy as np

from oracle.pyoracle import FR_MODULUS, aligned_empty, to_int

R = FR_MODULUS
MONT = (1 << 256) % R          # raw limbs of the scalar one
MONT_INV = pow(MONT, -1, R)

XS = ("one", "minus_one", "root4", "root8", "two")
MIXES = ("one_value", "alternating", "halves", "zero_pm1", "random", "zero_sum")
NMAX = 1 << 14
SEED = 0xC0111DE5


def x_raw(oracle, name):
    """the table's secret as raw Montgomery limbs (an int): what oracle.make_srs takes"""
    return {"one": MONT, "minus_one": R - MONT, "root4": to_int(oracle.root_of_unity(2)), "root8": to_int(oracle.root_of_unity(3)),
            "two": 2 * MONT % R}[name]


def x_plain(oracle, name):
    return x_raw(oracle, name) * MONT_INV % R


def seed_of(xname, mix, n):
    return SEED + (XS.index(xname) * len(MIXES) + MIXES.index(mix)) * 0x10001 + n


def to_limbs(values):
    """ints < 2^256 -> (n, 4) uint64, 64-byte aligned (the reference wants its scalars aligned)"""
    out = aligned_empty((len(values), 4))
    out[...] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4)
    return out


def _ints(arr):
    buf = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(buf[32 * i:32 * i + 32], "little") for i in range(arr.shape[0])]


def powers(x, n):
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * x % R
    return out


def raw_scalars(oracle, mix, n, x, seed):
    """the n raw scalars of a mix (ints in [0, r)); x is the table's plain secret (only zero_sum looks at it).

    What a mix reaches depends on the TABLE, because equal and opposite points only meet when they fall into one bucket, and a bucket is chosen
    by the scalar's window digits: the digits of r - s are NOT the negated digits of s (r is no multiple of 2^c), so s and -s go to different
    buckets with the same point sign.
      one_value    every entry has the same digits: one bucket per window holds the whole table.  On x = 1 that bucket holds n copies of one point:
                   every chunk of two or more entries doubles at its second entry, all full chunks leave the same partial, every level of
                   the merge tree is a doubling.  On x = -1 (root4, root8) the bucket holds a point and its negative in equal numbers: the sums
                   inside a chunk are k P with small k, so they double at k = +-1, cancel whenever k returns to 0 and restart from the flag; the
                   partials are small multiples of both signs and infinities, so the merges see equal, opposite and infinite operands.
      alternating, halves   s and r - s: two such buckets per window (on x = 1: two heavy buckets of equal points -- doublings and equal partials
                   only; the total reaches infinity in the final reduction, not in a chunk).  On x = -1 alternating puts all G under s and all
                   -G under r - s, halves puts both signs under each.
      zero_pm1     three values: buckets of a third of the table each in the lowest window, the digit 0 dropped.
      random       buckets of a few entries: on x = 1 every one of them is a doubling chain; on x = -1 signs mix inside them.
      zero_sum     random but for the last scalar, solved so that the result is the infinity flag on every table."""
    rnd = _ints(oracle.random_scalars(seed, n))  # canonical, non-zero with overwhelming probability
    s = rnd[0]
    if mix == "one_value":
        return [s] * n
    if mix == "alternating":
        return [s if i % 2 == 0 else R - s for i in range(n)]
    if mix == "halves":
        return [s if i < n // 2 else R - s for i in range(n)]
    if mix == "zero_pm1":
        return [(0, MONT, R - MONT)[v % 3] for v in rnd]
    if mix == "random":
        return rnd
    if mix == "zero_sum":
        pw = powers(x, n)
        head = sum(m * p for m, p in zip(rnd[:-1], pw[:-1])) % R
        return rnd[:-1] + [(-head) * pow(pw[-1], -1, R) % R]
    raise KeyError(mix)


def closed_form_scalar(raw, x):
    """sum m_i x^i mod r, raw form"""
    return sum(m * p for m, p in zip(raw, powers(x, len(raw)))) % R


def closed_form_point(oracle, k):
    """k G as the MSM entries return it: normalised (x, y, one) or the infinity flag"""
    from oracle.pyoracle import from_int
    return oracle.g1_scalar_mul(oracle.g1_one_affine(), from_int(k))


class Tables:
    """the nmax-point table of every x, built on first use and sliced for smaller n"""

    def __init__(self, oracle, nmax=NMAX):
        self.oracle, self.nmax, self._tab, self._cases = oracle, nmax, {}, {}

    def points(self, xname):
        """(plain points (nmax, 8), endomorphism table (2 nmax, 8))"""
        if xname not in self._tab:
            from oracle.pyoracle import from_int
            srs = self.oracle.make_srs(from_int(x_raw(self.oracle, xname)), self.nmax)
            self._tab[xname] = (srs, self.oracle.point_table(srs))
        return self._tab[xname]

    def case(self, xname, mix, n):
        """(scalars (n, 4) aligned, expected point (12,)) -- computed once, shared by every test that asks, never written to.  The expected
        point is the closed form; the oracle's Pippenger has to agree with it here, so that a later mismatch of the code under test is its own"""
        key = (xname, mix, n)
        if key not in self._cases:
            O = self.oracle
            x = x_plain(O, xname)
            raw = raw_scalars(O, mix, n, x, seed_of(xname, mix, n))
            k = closed_form_scalar(raw, x)
            assert k == 0 or mix != "zero_sum", key  # (other mixes cancel too where the table does it for them: one value on G, -G, G, ... with n even)
            want = closed_form_point(O, k)
            sc = to_limbs(raw)
            got = O.msm_affine(sc, self.points(xname)[1], n)
            assert np.array_equal(got, want), ("oracle.msm_affine disagrees with the closed form", key)
            sc.setflags(write=False)
            want.setflags(write=False)
            self._cases[key] = (sc, want)
        return self._cases[key]


def same_point(got, want, one=None):
    """x, y and the infinity bit exactly (limbs 0-7: the flag is bit 63 of y's top limb); z = one where the entry normalises"""
    if not np.array_equal(got[:8], want[:8]):
        return False
    return one is None or bool(int(want[7]) >> 63) or np.array_equal(got[8:12], one)
