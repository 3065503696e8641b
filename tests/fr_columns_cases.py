"""Shared cases of the column tests (tests/test_fr_columns_host.py, tests/test_gpu_fr_columns.py; test infrastructure, may import oracle/): row-major
matrices whose COLUMNS are codewords -- the values of seeded polynomials of degree < d on the size-`rows` domain --, the row sets a call lists (column j
uses set j mod sets), and a sentinel fill for the elements at [width, stride) of every row.  Small matrices are made over Python integers
(tests/kzg_recover_cells_cases.py: transform, interpolate), which share no code with the library.  Shapes too large for that are made from seeded
coefficient rows by bbgpu_host_fr_ntt_columns, which tests/test_fr_columns_host.py holds to bbgpu_host_ntt: such a matrix only has to BE a matrix of
codewords, what is checked on it is the device against the twin."""
import numpy as np

from oracle.pyoracle import FR_MODULUS as R, aligned_copy, from_int, to_int
from tests.kzg_recover_cells_cases import ERR_ARG, ERR_HIP, ERR_SIZE, interpolate, log2, memory, plain, transform  # noqa: F401

NONE = 0xFFFFFFFF         # an entry of first_bad where the column has none
SENTINEL = 0xA5A5A5A5A5A5A5A5  # every word of the elements at [width, stride)
JUNK = 0xFFFFFFFFFFFFFFFF      # every word of a missing element before the call: not a field element's canonical form, and never read
PAD = 5


def codeword_ints(rows, width, d, seed=0):
    """ints[r][j]: column j holds the values of a seeded polynomial of degree EXACTLY d - 1, over Python integers"""
    rng = np.random.default_rng([0xC01, rows, width, d, seed])
    out = [[0] * width for _ in range(rows)]
    for j in range(width):
        c = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(d)]
        c[-1] = c[-1] or 1
        for r, v in enumerate(transform(c, rows)):
            out[r][j] = v
    return out


def matrix_memory(ints, stride):
    """(rows * stride, 4) uint64 in the memory format, canonical; the elements at [width, stride) of every row hold the sentinel"""
    rows, width = len(ints), len(ints[0])
    mem = np.full((rows, stride, 4), SENTINEL, dtype=np.uint64)
    for r in range(rows):
        mem[r, :width] = memory(ints[r])
    return aligned_copy(mem.reshape(rows * stride, 4))


def random_elements(count, seed):
    """(count, 4) seeded canonical elements: the top limb below 2^61 keeps every one below r"""
    rng = np.random.default_rng([0xE1E, count, seed])
    out = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    out[:, 3] &= np.uint64((1 << 61) - 1)
    return out


def codeword_memory(lib, rows, width, d, stride, seed=0):
    """the same kind of matrix for large shapes: seeded coefficient rows [0, d), zero rows above, transformed down the columns by the host twin"""
    mem = np.full((rows, stride, 4), SENTINEL, dtype=np.uint64)
    mem[:, :width] = 0
    mem[:d, :width] = random_elements(d * width, seed).reshape(d, width, 4)
    mem = aligned_copy(mem.reshape(rows * stride, 4))
    lib.host_fr_ntt_columns(mem, rows, width, "fft", stride=stride)
    return mem


def row_sets(rows, mus, seed=7, shuffle=True):
    """per set the PRESENT rows (uint32), mus[s] of the rows missing: a different seeded set per s, in a seeded shuffled order (or ascending)"""
    out = []
    for s, mu in enumerate(mus):
        rng = np.random.default_rng([0x5E7, rows, mu, s, seed])
        present = np.sort(rng.permutation(rows)[mu:]).astype(np.uint32)
        if shuffle:
            rng.shuffle(present)
        out.append(present)
    return out


def missing_of(rows, present):
    gone = np.ones(rows, dtype=bool)
    gone[np.asarray(present, dtype=np.int64)] = False
    return np.nonzero(gone)[0]


def missing_mask(rows, width, sets_rows):
    """(rows, width) bool: True where column j's set misses row r"""
    mask = np.zeros((rows, width), dtype=bool)
    for s, present in enumerate(sets_rows):
        mask[np.ix_(missing_of(rows, present), np.arange(s, width, len(sets_rows)))] = True
    return mask


def erase(mem, rows, width, stride, sets_rows):
    """a copy of the matrix with every missing element overwritten by JUNK words: what the caller holds before the call"""
    out = mem.copy().reshape(rows, stride, 4)
    out[:, :width][missing_mask(rows, width, sets_rows)] = JUNK
    return aligned_copy(out.reshape(rows * stride, 4))


def element(mem, stride, r, j):
    return mem.reshape(-1, stride, 4)[r, j]


def alter(mem, stride, r, j, delta=1):
    """element (r, j) + delta in the field, canonical, in place"""
    mem.reshape(-1, stride, 4)[r, j] = memory([plain(element(mem, stride, r, j))[0] + delta])[0]


def add_modulus_where_it_fits(mem):
    """every element + r where that stays below 2^256: another representative; -> (the copy, how many elements changed)"""
    out, changed = mem.copy(), 0
    for i in range(out.shape[0]):
        v = to_int(out[i]) + R
        if v < 1 << 256:
            out[i] = from_int(v)
            changed += 1
    return out, changed


def clean_report(rows, sets_rows):
    return dict(consistent=1, first_bad_column=0, first_bad_coeff=0, max_missing=max(rows - len(p) for p in sets_rows))


def lagrange_column(rows, present, column_ints):
    """coefficients (rows of them) of the unique polynomial of degree < len(present) through the present rows of one column, and its values on the domain"""
    coeffs = interpolate(rows, 1, [int(k) for k in present], [column_ints[int(k)] for k in present])
    return coeffs, transform(coeffs, rows)


def expected_first_bad(rows, d, sets_rows, ints):
    """per column the smallest index in [d, count_s) with a nonzero coefficient of the interpolation, NONE for none -- the definition"""
    width, out = len(ints[0]), []
    for j in range(width):
        present = sets_rows[j % len(sets_rows)]
        coeffs, _ = lagrange_column(rows, present, [ints[r][j] for r in range(rows)])
        bad = [i for i in range(d, len(present)) if coeffs[i] % R]
        out.append(bad[0] if bad else NONE)
    return out


def report_of(first_bad, rows, sets_rows):
    rep = clean_report(rows, sets_rows)
    for j, v in enumerate(first_bad):
        if int(v) != NONE:
            rep.update(consistent=0, first_bad_column=j, first_bad_coeff=int(v))
            break
    return rep
