"""Shared cases of the bbgpu_g1_recover_each tests (tests/test_g1_recover_each_host.py, tests/test_gpu_g1_recover_each.py; test infrastructure, may import
oracle/): columns of points v_i * G as tests/g1_recover_cases.py makes them, every column with ITS OWN seeded set of present rows.  The statement on the
scalars that shares no code with the library: the decoder returns (the values of the column's polynomial) * G, and report and first_bad are the ones
bbgpu_host_kzg_recover_cells_each gives on the scalars at coset 1."""
import numpy as np

from tests.g1_recover_cases import (ERR_ARG, ERR_SIZE, INF, R, column_scalars, memory, missing_rows, output_buffer, points_of, present_rows,  # noqa: F401
                                    times_g)

NONE = 0xFFFFFFFFFFFFFFFF  # an entry of first_bad where the column has none


def column_rows(n, mus, seed=5, shuffle=True):
    """per column b the rows that are present, mus[b] of the n missing: a different seeded set per column, in a seeded shuffled order (or ascending)"""
    out = []
    for b, mu in enumerate(mus):
        rows = present_rows(n, missing_rows(n, mu, seed=seed + 16 * b), seed=seed + b)
        out.append(rows if shuffle else np.sort(rows))
    return out


def each_points(oracle, columns, rows):
    """the `points` argument as a list: (count_b, 8) per column, listed row t"""
    return [points_of(oracle, [vals[int(k)] for k in r]) for vals, r in zip(columns, rows)]


def each_scalars(columns, rows):
    """the `values` argument of the scalar decoder at coset 1 over the same columns and rows"""
    return [memory([vals[int(k)] for k in r]) for vals, r in zip(columns, rows)]


def scalar_each_report(lib, rows, values, n, d):
    """report and first_bad of bbgpu_host_kzg_recover_cells_each on the scalars at coset 1, in the names of bbgpu_g1_recover_each_report"""
    _, _, rep, first_bad = lib.host_kzg_recover_cells_each(rows, values, n, 1, d, want_values=False)
    return dict(consistent=rep["consistent"], first_bad_column=rep["first_bad_poly"], first_bad_coeff=rep["first_bad_coeff"],
                max_missing=rep["max_missing"]), first_bad


def each_case(oracle, n, d, mus, alter=(), edit=None, seed=5):
    """-> per-column rows, the columns' scalars (edit(cols, rows) first; then + 1, that is P + G, at listed position t of column b for every (b, t) of
    alter), the per-column points"""
    rows = column_rows(n, mus, seed=seed)
    cols = [list(v) for v in column_scalars(n, d, len(mus))]
    if edit:
        edit(cols, rows)
    for b, t in alter:
        cols[b][int(rows[b][t])] += 1
    return rows, cols, each_points(oracle, cols, rows)


def clean_report(mus):
    return dict(consistent=1, first_bad_column=0, first_bad_coeff=0, max_missing=max(mus))
