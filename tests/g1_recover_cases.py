"""Shared cases of the G1 transform and recover tests (tests/test_g1_recover_host.py, tests/test_gpu_g1_recover.py; test infrastructure, may import
oracle/).  A column of points is made from a column of SCALARS: P_i = v_i * G by the oracle's scalar multiplication.  G has prime order and the scalars are
canonical, so everything the library does to the points has a statement on the scalars that shares no code with it: the transform of the points is
(the transform of v over Python integers) * G, the decoder returns (the values of the polynomial) * G, and coefficient j of its D is at infinity iff the
scalar decoder's coefficient j is zero -- bbgpu_host_kzg_recover_cells at coset 1 gives the report."""
import numpy as np

from oracle.pyoracle import FR_MODULUS as R, PolyOracle, aligned_copy
from tests.kzg_recover_cells_cases import ERR_ARG, ERR_HIP, ERR_SIZE, interpolate, log2, memory, omega, polynomial, transform  # noqa: F401

INF = np.array([0, 0, 0, 0, 0, 0, 0, 1 << 63], dtype=np.uint64)
SHAPES = [(2, 1, 1), (8, 4, 4), (8, 4, 1), (64, 17, 30)]  # (n, d, missing)
_POINTS = {}


def times_g(oracle, v):
    """(8,) v * G in the reference's affine memory format, the flag of infinity for v = 0 mod r; cached: the cases share most of their scalars"""
    v %= R
    if v not in _POINTS:
        if v == 0:
            _POINTS[v] = INF.copy()
        else:
            p = oracle.g1_normalize_or_inf(oracle.g1_scalar_mul(oracle.g1_one_affine(), PolyOracle.mont([v])[0]))
            _POINTS[v] = np.array(p[:8], dtype=np.uint64)
    return _POINTS[v]


def points_of(oracle, scalars):
    """(len, 8) uint64: scalars[i] * G"""
    return aligned_copy(np.stack([times_g(oracle, int(v)) for v in scalars]))


def inverse_transform(v, n):
    """the coefficients of the values v on the size-n domain, over Python integers"""
    a = transform(list(v), n)
    ninv = pow(n, -1, R)
    return [a[(n - i) % n] * ninv % R for i in range(n)]


def present_rows(n, missing, seed=2):
    """the rows that are not missing, in a seeded shuffled order, as uint32"""
    gone = set(missing)
    rows = [k for k in range(n) if k not in gone]
    np.random.default_rng([0x61EC, n, len(missing), seed]).shuffle(rows)
    return np.array(rows, dtype=np.uint32)


def missing_rows(n, mu, seed=3):
    return sorted(int(k) for k in np.random.default_rng([0x61ED, n, mu, seed]).permutation(n)[:mu])


def column_scalars(n, d, batch):
    """batch value tuples: column b holds the values of polynomial b of degree exactly d - 1"""
    return [polynomial(n, d, b)[1] for b in range(batch)]


def call_points(oracle, columns, rows):
    """the `points` argument of one recover call, (batch * count, 8): column b, listed row t"""
    return points_of(oracle, [vals[int(k)] for vals in columns for k in rows])


def call_scalars(columns, rows):
    """the `values` argument of the scalar decoder at coset 1 over the same columns and rows"""
    return memory([vals[int(k)] for vals in columns for k in rows])


def scalar_report(lib, rows, values, n, d, batch):
    """the report of bbgpu_host_kzg_recover_cells on the scalars at coset 1, in the names of bbgpu_g1_recover_report"""
    _, _, rep = lib.host_kzg_recover_cells(rows, values, n, 1, d, batch=batch, want_values=False)
    return dict(consistent=rep["consistent"], first_bad_column=rep["first_bad_poly"], first_bad_coeff=rep["first_bad_coeff"], missing=rep["missing"])


def output_buffer(batch, n, seed=0xF112):
    """(batch, n, 8) of other values: what a call's output lies in, so that untouched words show"""
    rng = np.random.default_rng(seed)
    return aligned_copy(rng.integers(0, 1 << 63, size=(batch, n, 8), dtype=np.uint64))


def extended_world(lib, oracle, tmp_path, n=256, l=4, k=4):
    """a 2-D layout: k random polynomials of degree < n extended column-wise to R = 2 k rows by the SCALAR transform (every coefficient index is a column:
    size-k inverse, then size-2k forward over the zero-padded column), and the world of tests/kzg_check_cells_cases.py over the R rows -- commitments
    (R, 8), proofs (R, n / l, 8), values.  Even rows are the original polynomials.  -> (world, columns (1 + n / l, R, 8): the commitments' column, then
    one column per cell)"""
    from tests.kzg_check_cells_cases import make_world
    base = [[int(x) for x in PolyOracle.plain(oracle.random_scalars(0x2D00 + r, n))] for r in range(k)]
    rows = [[0] * n for _ in range(2 * k)]
    for c in range(n):
        ext = transform(inverse_transform([base[r][c] for r in range(k)], k), 2 * k)
        for r in range(2 * k):
            rows[r][c] = ext[r]
    assert all(rows[2 * r] == base[r] for r in range(k))
    W = make_world(lib, oracle, tmp_path, n, l, 2 * k, coeffs=np.stack([memory(r) for r in rows]))
    columns = np.concatenate([W["commitments"][None, :, :], W["proofs"].transpose(1, 0, 2)])
    return W, aligned_copy(columns)
