"""Shared cases of the SRS-update tests (tests/test_srs_update_host.py, tests/test_gpu_srs_update.py; test infrastructure, may import oracle/): the secrets,
the tables and what an update must give.  Every expected value is the oracle's: make_srs(x y, n) is, bit for bit, the update by y of make_srs(x, n);
msm_affine([k], [P]) is k P for one row; mul(FR, ., .) gives the products of secrets.  The host and the GPU entry are judged against the same values."""
import numpy as np

from oracle.pyoracle import FR, FR_MODULUS as R, aligned_copy, from_int, to_int

NONE = 0xFFFFFFFFFFFFFFFF
X_SEED, Y_SEED, OTHER_SEED = 0xC0FFEE, 0x5EC2E7, 0x0DDBA11
# the constants of the endomorphism split (field.hpp:420-426): c1 = (g2 k) >> 256, c2 = (g1 k) >> 256, t = c2 b2 - c1 (-b1)
G2_WINDOW = (2 << 64) | 0xD91D232EC7E0B3D7
G1_WINDOW = (2 << 128) | (0x4CCEF014A773D2CF << 64) | 0x7A7BD9D4391EB18D
MINUS_B1 = (0x6F4D8248EEB859FC << 64) | 0x8211BBEB7D4F1128
B2 = 0x89D3256894D213E3


def lam(oracle):
    """the cube root of unity the split uses, as a plain integer"""
    return to_int(oracle.from_mont(FR, oracle.const(FR, "beta")))


def mont(oracle, v):
    return oracle.to_mont(FR, from_int(v % R))


def secret_x(oracle):
    return oracle.random_scalars(X_SEED, 1)[0]


def secret_y(oracle):
    return oracle.random_scalars(Y_SEED, 1)[0]


def special_ys(oracle):
    """(name, y in Montgomery form): the scalars that reach every case of the ladder's additions and of the split.  Small y: the accumulator starts at
    infinity and k2 = 0 adds and takes away the image point; lambda +- 1, r - lambda: one half is 0 or 1 and the two halves cancel or double; r - 1, r - 2:
    both halves full; 2^128: the first scalar whose k1 needs the split at all; y + r: a representative that is not canonical; ceil(2^256 / g2): the first
    scalar for which the split's t is NEGATIVE (the floors of c1 and c2 leave t = c2 b2 - c1 (-b1) below zero just above a multiple of 2^256 / g2)."""
    y = secret_y(oracle)
    L = lam(oracle)
    out = [("random", y), ("one", mont(oracle, 1)), ("two", mont(oracle, 2)), ("three", mont(oracle, 3)), ("r-1", mont(oracle, R - 1)),
           ("r-2", mont(oracle, R - 2)), ("lambda", mont(oracle, L)), ("lambda+1", mont(oracle, L + 1)), ("lambda-1", mont(oracle, L - 1)),
           ("r-lambda", mont(oracle, R - L)), ("2^128", mont(oracle, 1 << 128)), ("random+r", from_int(to_int(y) + R)),
           ("negative-t", mont(oracle, -((-(1 << 256)) // G2_WINDOW)))]
    assert to_int(out[11][1]) < 1 << 256
    return out


def honest_table(oracle, x, n):
    return oracle.point_table(oracle.make_srs(x, n))


def all_g_table(oracle, n):
    """the table of x = 1: every row is the generator"""
    return oracle.point_table(oracle.make_srs(oracle.const(FR, "one"), n))


def unrelated_points(oracle, n):
    """on-curve rows that are no chain of powers from the generator: the rows of another secret's string in reversed order"""
    return aligned_copy(oracle.make_srs(oracle.random_scalars(OTHER_SEED, 1)[0], n + 1)[::-1][:n])


def updated_table(oracle, x, y, n):
    """the update by y of the honest table of x"""
    return oracle.point_table(oracle.make_srs(oracle.mul(FR, x, y), n))


def row_times(oracle, point8, k_mont):
    """k P for one affine row, (8,): the oracle's MSM of one point"""
    p = aligned_copy(np.asarray(point8, dtype=np.uint64).reshape(1, 8))
    return oracle.msm_affine(aligned_copy(np.asarray(k_mont, dtype=np.uint64).reshape(1, 4)), oracle.point_table(p), 1)[:8]


def row_times_plain(oracle, point8, k_mont):
    """the same by the oracle's plain scalar multiplication, without the endomorphism split.  For the scalars whose split has a negative t the oracle's MSM
    -- like the reference's, whose split it restates -- takes the low limbs of r - |t| for k2 and returns another point; this one is k P for every k"""
    return oracle.g1_normalize(oracle.g1_scalar_mul(np.asarray(point8, dtype=np.uint64).reshape(8), k_mont))[:8]


def rows_times_powers(oracle, points, y, first=0):
    """the endo table of y^(first + i) P_i, row by row through the oracle's MSM of one point"""
    n = points.shape[0]
    out = np.zeros((n, 8), dtype=np.uint64)
    k = mont(oracle, 1)
    for _ in range(first):
        k = oracle.mul(FR, k, y)
    for i in range(n):
        out[i] = row_times(oracle, points[i], k)
        k = oracle.mul(FR, k, y)
    return oracle.point_table(aligned_copy(out))


def tampered(table, k):
    """one added to the y of row k: off the curve"""
    t = aligned_copy(table)
    t[2 * k, 4:8] = from_int((to_int(t[2 * k, 4:8]) + 1) % (1 << 256))
    return t


def split_cases(oracle, golden):
    """scalars for the split self-test: the golden ones (with the split they must give), the special ones, 40 scalars just above multiples of 2^256 / g2
    (negative t) and 200 random ones"""
    cases = golden("endo_wnaf.json")["cases"]
    pinned = [(to_int([int(v, 16) for v in c["k"]]), to_int([int(v, 16) for v in c["k1"]]), to_int([int(v, 16) for v in c["k2"]])) for c in cases]
    L = lam(oracle)
    free = [1, 2, 3, R - 1, R - 2, L, L + 1, L - 1, R - L, 1 << 128, (1 << 128) - 1, R, R + 5, (1 << 256) - 1]
    free += [-((-(j << 256)) // G2_WINDOW) + d for j in range(1, 21) for d in (0, 1)]
    free += [to_int(v) for v in oracle.random_scalars(0x5B117, 200)]
    return pinned, free


def check_split(oracle, pinned, free, out):
    """out: the (n, 6) result of bbgpu_selftest_endo_split over pinned + free, in that order.  The golden scalars give the golden split; every other one
    gives the split the formula defines over the integers (t signed, k1 the residue of k + t lambda nearest zero), and that is a split of k"""
    L = lam(oracle)
    negatives = 0
    for i, (k, k1, k2) in enumerate(pinned):
        assert [to_int(out[i, 0:2]), to_int(out[i, 2:4]), int(out[i, 4])] == [k1, k2, 0], hex(k)
    for j, k in enumerate(free):
        row = out[len(pinned) + j]
        flags = int(row[4])
        t = ((G1_WINDOW * k) >> 256) * B2 - ((G2_WINDOW * k) >> 256) * MINUS_B1
        k1 = (k + t * L) % R
        k1 = k1 - R if k1 > R // 2 else k1
        assert abs(k1) < 1 << 128 and abs(t) < 1 << 128 and (k1 - L * t - k) % R == 0, hex(k)
        assert [to_int(row[0:2]), to_int(row[2:4]), flags] == [abs(k1), abs(t), (1 if k1 < 0 else 0) | (2 if t < 0 else 0)], hex(k)
        negatives += 1 if t < 0 else 0
    assert negatives >= 1  # the scalars chosen for a negative t have one
