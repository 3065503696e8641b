"""bbgpu_host_g1_recover_each (csrc/host_g1_recover.hpp g1_recover_each_host): the erasure decoder in the group for columns whose row sets DIFFER, held to
statements that share no code with it -- columns of multiples v_i * G of the generator (tests/g1_recover_each_cases.py): the decoder returns every v_i * G
of the column's polynomial, and its report and first_bad are the ones bbgpu_host_kzg_recover_cells_each gives on the scalars at coset 1; where every
column lists the same rows it equals bbgpu_host_g1_recover bit for bit.  Then altered points with and without redundancy, and every refusal of
include/bbgpu.h through the twin and through the device entry on a machine without a GPU.  The twin is what the GPU entry is compared with bit for bit
(tests/test_gpu_g1_recover_each.py).  CPU tests."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.g1_recover_each_cases import (ERR_ARG, ERR_SIZE, NONE, clean_report, column_scalars, each_case, each_points, each_scalars, output_buffer,
                                         points_of, scalar_each_report)
from tests.test_g1_recover_host import flagged, not_canonical, off_curve

SHAPES = [(2, 1, (1, 0, 1)), (8, 4, (0, 1, 2, 3, 4)), (64, 17, (0, 1, 30, 47))]  # (n, d, missing per column)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.mark.parametrize("n,d,mus", SHAPES)
def test_twin_recovers_every_point_of_every_column(lib, oracle, n, d, mus):
    rows, cols, points = each_case(oracle, n, d, mus)
    kept = [p.copy() for p in points]
    got, rep, first_bad = lib.host_g1_recover_each(rows, points, n, d)
    want_rep, want_bad = scalar_each_report(lib, rows, each_scalars(cols, rows), n, d)
    assert all(np.array_equal(p, k) for p, k in zip(points, kept))
    assert rep == want_rep == clean_report(mus) and np.array_equal(first_bad, want_bad) and all(int(v) == NONE for v in first_bad)
    for b, col in enumerate(cols):
        assert np.array_equal(got[b], points_of(oracle, col)), b
    flat = np.concatenate(points)  # one array in the order of the lists is the same call
    again, rep2, bad2 = lib.host_g1_recover_each(rows, flat, n, d)
    assert np.array_equal(again, got) and rep2 == rep and np.array_equal(bad2, first_bad)


@pytest.mark.parametrize("n,d,mu,batch", [(8, 4, 3, 3), (64, 17, 30, 2)])
@pytest.mark.parametrize("shuffled", [False, True])
def test_the_same_rows_in_every_column_equal_the_same_set_twin(lib, oracle, n, d, mu, batch, shuffled):
    """one set for all columns: in the same order in every column, and in per-column shuffled orders of that set"""
    from tests.g1_recover_cases import call_points, missing_rows, present_rows
    gone = missing_rows(n, mu)
    shared = present_rows(n, gone)
    cols = [list(v) for v in column_scalars(n, d, batch)]
    want, want_rep = lib.host_g1_recover(shared, call_points(oracle, cols, shared), n, d, batch=batch)
    rows = [present_rows(n, gone, seed=40 + b) if shuffled else shared for b in range(batch)]
    assert not shuffled or any(not np.array_equal(r, shared) for r in rows)
    got, rep, first_bad = lib.host_g1_recover_each(rows, each_points(oracle, cols, rows), n, d)
    assert np.array_equal(got, want) and all(int(v) == NONE for v in first_bad)
    assert rep == dict(consistent=want_rep["consistent"], first_bad_column=want_rep["first_bad_column"], first_bad_coeff=want_rep["first_bad_coeff"],
                       max_missing=want_rep["missing"]) == clean_report([mu])


def test_an_altered_point_names_its_column_and_leaves_the_others_exact(lib, oracle):
    n, d, mus = 8, 4, (0, 1, 2, 3, 4)
    rows, cols, points = each_case(oracle, n, d, mus, alter=[(2, 1)])  # column 2 has 6 rows for degree < 4
    got, rep, first_bad = lib.host_g1_recover_each(rows, points, n, d)
    want_rep, want_bad = scalar_each_report(lib, rows, each_scalars(cols, rows), n, d)
    assert rep == want_rep and np.array_equal(first_bad, want_bad)
    assert rep["consistent"] == 0 and rep["first_bad_column"] == 2 and d <= rep["first_bad_coeff"] < n - 2 and rep["max_missing"] == 4
    assert [int(v) != NONE for v in first_bad] == [False, False, True, False, False] and int(first_bad[2]) == rep["first_bad_coeff"]
    clean = column_scalars(n, d, len(mus))
    for b in (0, 1, 3, 4):
        assert np.array_equal(got[b], points_of(oracle, clean[b])), b


def test_two_altered_columns_the_report_names_the_first_and_first_bad_shows_both(lib, oracle):
    n, d, mus = 8, 4, (0, 1, 2, 3, 4)
    rows, cols, points = each_case(oracle, n, d, mus, alter=[(3, 0), (1, 4)])  # column 3 has 5 rows, column 1 has 7
    got, rep, first_bad = lib.host_g1_recover_each(rows, points, n, d)
    want_rep, want_bad = scalar_each_report(lib, rows, each_scalars(cols, rows), n, d)
    assert rep == want_rep and np.array_equal(first_bad, want_bad)
    assert rep["consistent"] == 0 and rep["first_bad_column"] == 1 and rep["first_bad_coeff"] == int(first_bad[1])
    assert [int(v) != NONE for v in first_bad] == [False, True, False, True, False]
    assert d <= int(first_bad[1]) < 7 and int(first_bad[3]) == 4  # column 3: [d, count) is the one index 4


def test_an_alteration_where_the_count_is_the_degree_bound_is_not_seen(lib, oracle):
    n, d, mus = 8, 4, (0, 1, 2, 3, 4)
    rows, cols, points = each_case(oracle, n, d, mus, alter=[(4, 2)])  # column 4 lists exactly d rows
    got, rep, first_bad = lib.host_g1_recover_each(rows, points, n, d)
    want_rep, want_bad = scalar_each_report(lib, rows, each_scalars(cols, rows), n, d)
    assert rep == want_rep == clean_report(mus) and np.array_equal(first_bad, want_bad) and all(int(v) == NONE for v in first_bad)
    for t, k in enumerate(rows[4]):  # the column is still written: it passes through the listed points as they were given
        assert np.array_equal(got[4][int(k)], points[4][t])


GOOD_ROWS = ([0, 1, 2, 3, 4, 5], [7, 6, 5, 4, 3])


def refusals(oracle):
    """(kwargs, verdict, text) for every refusal of bbgpu_g1_recover_each; everything defaults to a good call at n = 8, d = 4, rows 0 .. 5 and 7 .. 3"""
    out = [(dict(n=0), ERR_SIZE, "power of two"), (dict(n=1), ERR_SIZE, "power of two"), (dict(n=12), ERR_SIZE, "power of two"),
           (dict(n=1 << 13), ERR_SIZE, r"between 2 and 2\^12"), (dict(d=0), ERR_SIZE, "degree bound 0"), (dict(d=9), ERR_SIZE, "degree bound 9"),
           (dict(batch=0), ERR_SIZE, "batch 0"), (dict(n=1 << 12, d=1, batch=257), ERR_SIZE, "batch x n"),
           (dict(d=6), ERR_SIZE, "column 1 lists 5 rows"), (dict(rows=(list(range(8)) + [0], GOOD_ROWS[1])), ERR_SIZE, "column 0 lists 9 rows"),
           (dict(offsets=[1, 6, 11]), ERR_ARG, r"row_offsets\[0\] = 1 is not 0"),
           (dict(offsets=[0, 6, 5]), ERR_ARG, r"column 1: row_offsets\[2\] = 5 is below row_offsets\[1\] = 6"),
           (dict(rows=(GOOD_ROWS[0], [7, 6, 8, 4, 3])), ERR_ARG, r"column 1: row\[8\] = 8 \(position 2 of its list\) is not below n = 8"),
           (dict(rows=(GOOD_ROWS[0], [7, 6, 5, 6, 3])), ERR_ARG, r"column 1: row\[9\] = 6 \(position 3 of its list\) is listed twice")]
    for bad in (off_curve(oracle), not_canonical(oracle), flagged(oracle)):
        out.append((dict(bad=(9, bad)), ERR_ARG, r"position 3 of column 1 \(row 4\) is not on the curve or not canonical"))
    return out


def raw_each(lib, fn, offsets, row, points, n, d, batch, out, first_bad, rep, *extra):
    from barretenberg_amd.bbgpu import G1RecoverEachReport, _ptr, u64p
    u32p = C.POINTER(C.c_uint32)
    fn.argtypes = [u32p, u32p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, C.POINTER(G1RecoverEachReport)] + [C.c_void_p] * len(extra)
    return fn(offsets.ctypes.data_as(u32p) if offsets is not None else None, row.ctypes.data_as(u32p) if row is not None else None,
              _ptr(points) if points is not None else None, n, d, batch, _ptr(out) if out is not None else None,
              _ptr(first_bad) if first_bad is not None else None, C.byref(rep) if rep is not None else None, *extra)


@pytest.mark.parametrize("device", [False, True])
def test_refusals_leave_the_outputs_untouched(lib, oracle, device):
    """every refusal of include/bbgpu.h, through the twin and through bbgpu_g1_recover_each on a machine without a GPU: nothing is initialised for a refused
    call; the message names the column and the position"""
    from barretenberg_amd.bbgpu import G1RecoverEachReport
    fn, extra = (lib.lib.bbgpu_g1_recover_each, (None,)) if device else (lib.lib.bbgpu_host_g1_recover_each, ())
    for kw, verdict, text in refusals(oracle):
        lists = kw.get("rows", GOOD_ROWS)
        row = np.array([k for r in lists for k in r], dtype=np.uint32)
        offsets = np.array(kw.get("offsets", [0, len(lists[0]), len(row)]), dtype=np.uint32)
        points = points_of(oracle, list(range(1, len(row) + 1)))
        if "bad" in kw:
            points[kw["bad"][0]] = kw["bad"][1]
        out, rep, first_bad = output_buffer(2, 8), G1RecoverEachReport(7, 7, 7, 7), np.full(2, 7, dtype=np.uint64)
        kept = out.copy()
        rc = raw_each(lib, fn, offsets, row, points, kw.get("n", 8), kw.get("d", 4), kw.get("batch", 2), out, first_bad, rep, *extra)
        err = lib.lib.bbgpu_last_error().decode()
        assert " %d:" % rc == verdict and re.search(text, err) and np.array_equal(out, kept), (kw, rc, err)
        assert rep.as_dict() == dict(consistent=7, first_bad_column=7, first_bad_coeff=7, max_missing=7) and list(first_bad) == [7, 7], kw
    row = np.array([k for r in GOOD_ROWS for k in r], dtype=np.uint32)
    offsets, points = np.array([0, 6, 11], dtype=np.uint32), points_of(oracle, list(range(1, 12)))
    for hole in range(5):
        out, rep = output_buffer(2, 8), G1RecoverEachReport(7, 7, 7, 7)
        kept = out.copy()
        args = [offsets, row, points, out, rep]
        args[hole] = None
        rc = raw_each(lib, fn, args[0], args[1], args[2], 8, 4, 2, args[3], None, args[4], *extra)
        assert rc == -3 and "null" in lib.lib.bbgpu_last_error().decode() and np.array_equal(out, kept), hole
    if not device:  # first_bad_out may be NULL: the call itself is good
        out, rep = output_buffer(2, 8), G1RecoverEachReport(7, 7, 7, 7)
        assert raw_each(lib, fn, offsets, row, points, 8, 4, 2, out, None, rep) == 0 and rep.max_missing == 3


def test_host_twin_under_sanitizers(tmp_path):
    """tests/cpp/test_g1_recover_each_host.cpp: the twin as a stand-alone program (own main) built with -fsanitize=address,undefined, at (8, 4) and (64, 17)
    with per-column sets: recovery of multiples of the generator, an altered point with and without redundancy, refused calls"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_g1_recover_each_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_g1_recover_each_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
