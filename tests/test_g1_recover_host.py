"""bbgpu_host_g1_ntt and bbgpu_host_g1_recover (csrc/host_g1_recover.hpp): transforms whose elements are curve points, and the erasure decoder in the
group, held to an independent statement on SCALARS -- columns of multiples v_i * G of the generator, made by the oracle's scalar multiplication
(tests/g1_recover_cases.py): the transform of the points is (the transform of v over Python integers) * G, the decoder returns every v_i * G, and its
report is the one bbgpu_host_kzg_recover_cells gives on the scalars at coset 1; at n <= 8 also Lagrange interpolation over Python integers.  Then altered
points, degenerate columns (all points equal, all at infinity, infinity among the present rows), and the argument verdicts of the twins and of the device
entries on a machine without a GPU.  The twins are what the GPU entries are compared with bit for bit (tests/test_gpu_g1_recover.py).  CPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FQ_MODULUS, from_int, to_int
from tests.g1_recover_cases import (ERR_ARG, ERR_SIZE, INF, R, SHAPES, call_points, call_scalars, column_scalars, interpolate, inverse_transform, memory,
                                    missing_rows, omega, output_buffer, points_of, present_rows, scalar_report, times_g, transform)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.mark.parametrize("n", [2, 8, 64])
@pytest.mark.parametrize("kind", ["fft", "ifft"])
def test_twin_transform_is_the_scalar_transform_times_the_generator(lib, oracle, n, kind):
    batch = 2
    cols = [list(v) for v in column_scalars(n, n, batch)]  # n values of a polynomial of full degree: nothing special about them
    points = points_of(oracle, [v for col in cols for v in col])
    kept = points.copy()
    got = lib.host_g1_ntt(points, n, kind, batch=batch)
    assert np.array_equal(points, kept)
    for b, col in enumerate(cols):
        want = transform(col, n) if kind == "fft" else inverse_transform(col, n)
        assert np.array_equal(got[b], points_of(oracle, want)), (n, kind, b)
    again = lib.host_g1_ntt(points, n, kind, batch=batch, out=points.reshape(batch, n, 8))  # in place
    assert np.array_equal(again, got)


def recover_case(oracle, n, d, mu, batch, alter=None):
    """-> rows, the columns' scalars (altered: + 1 at listed position alter[1] of column alter[0]), the points and the scalar decoder's values"""
    rows = present_rows(n, missing_rows(n, mu))
    cols = [list(v) for v in column_scalars(n, d, batch)]
    if alter is not None:
        cols[alter[0]][int(rows[alter[1]])] += 1  # P_i + G
    return rows, cols, call_points(oracle, cols, rows), call_scalars(cols, rows)


@pytest.mark.parametrize("n,d,mu", SHAPES)
def test_twin_recovers_every_point(lib, oracle, n, d, mu):
    batch = 2
    rows, cols, points, scalars = recover_case(oracle, n, d, mu, batch)
    kept = points.copy()
    got, rep = lib.host_g1_recover(rows, points, n, d, batch=batch)
    assert np.array_equal(points, kept)
    assert rep == scalar_report(lib, rows, scalars, n, d, batch) == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, missing=mu)
    for b, col in enumerate(cols):
        assert np.array_equal(got[b], points_of(oracle, col)), b
        if n <= 8:  # the polynomial through the listed values by Lagrange's formula, which never forms a vanishing polynomial
            c = interpolate(n, 1, rows, [col[int(k)] for k in rows])
            assert np.array_equal(got[b], points_of(oracle, transform(c, n))), b


def test_one_altered_point_among_redundant_rows(lib, oracle):
    n, d, mu, batch = 8, 4, 1, 3
    rows, cols, points, scalars = recover_case(oracle, n, d, mu, batch, alter=(1, 2))
    got, rep = lib.host_g1_recover(rows, points, n, d, batch=batch)
    want = scalar_report(lib, rows, scalars, n, d, batch)
    c = interpolate(n, 1, rows, [cols[1][int(k)] for k in rows])
    bad = [j for j in range(d, n - mu) if c[j]]
    assert bad and rep == want == dict(consistent=0, first_bad_column=1, first_bad_coeff=bad[0], missing=mu)
    # an inconsistent column is still written: the values of the polynomial of degree < count through the listed points
    assert np.array_equal(got[1], points_of(oracle, transform(c, n)))
    assert np.array_equal(got[0], points_of(oracle, cols[0])) and np.array_equal(got[2], points_of(oracle, cols[2]))


def test_the_same_alteration_without_redundancy_is_not_seen(lib, oracle):
    n, d, mu, batch = 8, 4, 4, 3
    rows, cols, points, scalars = recover_case(oracle, n, d, mu, batch, alter=(1, 2))
    got, rep = lib.host_g1_recover(rows, points, n, d, batch=batch)
    assert rep == scalar_report(lib, rows, scalars, n, d, batch) == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, missing=mu)
    c = interpolate(n, 1, rows, [cols[1][int(k)] for k in rows])
    assert np.array_equal(got[1], points_of(oracle, transform(c, n)))


def degenerate_columns(n=8):
    """{name: (scalars of the column, degree bound)}: n equal points (D = (P, inf, ..): every butterfly meets a doubling or a cancellation); all at
    infinity; a polynomial of degree 3 with a root ON the domain, so that a present row holds infinity"""
    x, c = pow(omega(n), 5, R), [0x1234567, 0x89ABCDE, 0xF012345, 0x6789ABC]
    c[0] = (c[0] - sum(ci * pow(x, i, R) for i, ci in enumerate(c))) % R
    rooted = transform(c, n)
    assert rooted[5] == 0 and all(rooted[i] for i in range(n) if i != 5)
    return {"equal": ([0xC0FFEE] * n, 1), "infinity": ([0] * n, 4), "root": (rooted, 4)}


@pytest.mark.parametrize("name", ["equal", "infinity", "root"])
def test_degenerate_columns(lib, oracle, name):
    n = 8
    col, d = degenerate_columns(n)[name]
    points = points_of(oracle, col)
    coeffs = inverse_transform(col, n)
    assert np.array_equal(lib.host_g1_ntt(points, n, "ifft")[0], points_of(oracle, coeffs))
    assert np.array_equal(lib.host_g1_ntt(points, n, "fft")[0], points_of(oracle, transform(col, n)))
    rows = np.array([5, 0, 7, 2, 3], dtype=np.uint32)  # row 5 listed: the infinity of "root" is among the present points
    got, rep = lib.host_g1_recover(rows, points[rows], n, d)
    assert rep == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, missing=3) and np.array_equal(got[0], points)
    if name != "equal":
        assert np.array_equal(points[5], INF)


def off_curve(oracle):
    p = times_g(oracle, 5).copy()
    p[:4], p[4:] = p[4:].copy(), p[:4].copy()  # (y, x): canonical coordinates, not on the curve
    return p


def not_canonical(oracle):
    p = times_g(oracle, 5).copy()
    p[:4] = from_int(to_int(p[:4]) + FQ_MODULUS)  # the same x, another representative below 2^256
    return p


def flagged(oracle):
    p = times_g(oracle, 5).copy()
    p[7] |= np.uint64(1 << 63)  # the flag of infinity over other words
    return p


def ntt_refusals(oracle):
    """(kwargs, verdict, text) for every refusal of bbgpu_g1_ntt; everything defaults to a good call at n = 8, batch 2"""
    out = [(dict(n=0), ERR_SIZE, "power of two"), (dict(n=1), ERR_SIZE, "power of two"), (dict(n=12), ERR_SIZE, "power of two"),
           (dict(n=1 << 17), ERR_SIZE, "power of two"), (dict(batch=0), ERR_SIZE, r"batch \(0\)"), (dict(n=1 << 16, batch=17), ERR_SIZE, "batch x n"),
           (dict(n=2, batch=(1 << 19) + 1), ERR_SIZE, "batch x n"),
           (dict(kind="coset_fft"), ERR_ARG, "kind 2"), (dict(kind="coset_ifft"), ERR_ARG, "kind 3"), (dict(kind="fft_with_constant"), ERR_ARG, "kind 4")]
    for name, bad in (("off", off_curve(oracle)), ("rep", not_canonical(oracle)), ("flag", flagged(oracle))):
        out.append((dict(bad=(11, bad)), ERR_ARG, "position 3 of column 1 is not on the curve or not canonical"))
    return out


def ntt_refusal_call(oracle, kw):
    n, batch = kw.get("n", 8), kw.get("batch", 2)
    points = points_of(oracle, list(range(1, 17)))  # sizes are judged before anything is read: no refused call needs more
    if "bad" in kw:
        points[kw["bad"][0]] = kw["bad"][1]
    return points, n, batch, kw.get("kind", "fft")


def raw_ntt(lib, fn, points, out, n, batch, kind, *extra):
    from barretenberg_amd.bbgpu import NTT_KINDS, _ptr, u64p
    fn.argtypes = [u64p, u64p, C.c_size_t, C.c_int, C.c_int] + [C.c_void_p] * len(extra)
    return fn(_ptr(points) if points is not None else None, _ptr(out) if out is not None else None, n, batch, NTT_KINDS[kind], *extra)


@pytest.mark.parametrize("device", [False, True])
def test_transform_refusals_leave_the_output_untouched(lib, oracle, device):
    """every refusal of include/bbgpu.h, through the twin and through bbgpu_g1_ntt on a machine without a GPU: nothing is initialised for a refused call"""
    import re
    fn, extra = (lib.lib.bbgpu_g1_ntt, (None,)) if device else (lib.lib.bbgpu_host_g1_ntt, ())
    for kw, verdict, text in ntt_refusals(oracle):
        points, n, batch, kind = ntt_refusal_call(oracle, kw)
        out = output_buffer(2, 8)
        kept = out.copy()
        rc = raw_ntt(lib, fn, points, out, n, batch, kind, *extra)
        err = lib.lib.bbgpu_last_error().decode()
        assert " %d:" % rc == verdict and re.search(text, err) and np.array_equal(out, kept), (kw, rc, err)
    points = points_of(oracle, list(range(1, 17)))
    for a, b in ((None, points.copy()), (points, None)):
        assert raw_ntt(lib, fn, a, b, 8, 2, "fft", *extra) == -3 and "null" in lib.lib.bbgpu_last_error().decode()


def recover_refusals(oracle):
    """(kwargs, verdict, text) for every refusal of bbgpu_g1_recover; everything defaults to a good call at n = 8, d = 4, rows 0 .. 5, batch 2"""
    out = [(dict(n=0), ERR_SIZE, "power of two"), (dict(n=1), ERR_SIZE, "power of two"), (dict(n=12), ERR_SIZE, "power of two"),
           (dict(n=1 << 17), ERR_SIZE, "power of two"), (dict(d=0), ERR_SIZE, "degree bound 0"), (dict(d=9), ERR_SIZE, "degree bound 9"),
           (dict(d=7), ERR_SIZE, "6 rows"), (dict(rows=list(range(8)) + [0]), ERR_SIZE, "9 rows"), (dict(batch=0), ERR_SIZE, "batch 0"),
           (dict(n=1 << 16, d=1, batch=17), ERR_SIZE, "batch x n"),
           (dict(rows=[0, 1, 2, 3, 8, 5]), ERR_ARG, r"row\[4\] = 8 is not below n = 8"), (dict(rows=[0, 1, 2, 3, 1, 5]), ERR_ARG, r"row\[4\] = 1 is listed twice")]
    for bad in (off_curve(oracle), not_canonical(oracle), flagged(oracle)):
        out.append((dict(bad=(9, bad)), ERR_ARG, r"position 3 of column 1 \(row 3\) is not on the curve or not canonical"))
    return out


def raw_recover(lib, fn, rows, points, n, d, batch, out, rep, *extra):
    from barretenberg_amd.bbgpu import G1RecoverReport, _ptr, u64p
    u32p = C.POINTER(C.c_uint32)
    fn.argtypes = [u32p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, C.POINTER(G1RecoverReport)] + [C.c_void_p] * len(extra)
    return fn(rows.ctypes.data_as(u32p) if rows is not None else None, 6 if rows is None else rows.shape[0], _ptr(points) if points is not None else None, n, d,
              batch, _ptr(out) if out is not None else None, C.byref(rep) if rep is not None else None, *extra)


@pytest.mark.parametrize("device", [False, True])
def test_recover_refusals_leave_the_outputs_untouched(lib, oracle, device):
    import re
    from barretenberg_amd.bbgpu import G1RecoverReport
    fn, extra = (lib.lib.bbgpu_g1_recover, (None,)) if device else (lib.lib.bbgpu_host_g1_recover, ())
    for kw, verdict, text in recover_refusals(oracle):
        rows = np.array(kw.get("rows", [0, 1, 2, 3, 4, 5]), dtype=np.uint32)
        points = points_of(oracle, list(range(1, 2 * len(rows) + 1)))
        if "bad" in kw:
            points[kw["bad"][0]] = kw["bad"][1]
        out, rep = output_buffer(2, 8), G1RecoverReport(7, 7, 7, 7)
        kept = out.copy()
        rc = raw_recover(lib, fn, rows, points, kw.get("n", 8), kw.get("d", 4), kw.get("batch", 2), out, rep, *extra)
        err = lib.lib.bbgpu_last_error().decode()
        assert " %d:" % rc == verdict and re.search(text, err) and np.array_equal(out, kept), (kw, rc, err)
        assert rep.as_dict() == dict(consistent=7, first_bad_column=7, first_bad_coeff=7, missing=7), kw
    rows, points, out, rep = np.arange(6, dtype=np.uint32), points_of(oracle, list(range(1, 13))), output_buffer(2, 8), G1RecoverReport()
    for hole in range(4):
        args = [rows, points, out, rep]
        args[hole] = None
        assert raw_recover(lib, fn, args[0], args[1], 8, 4, 2, args[2], args[3], *extra) == -3 and "null" in lib.lib.bbgpu_last_error().decode(), hole


def test_commitments_and_proofs_of_a_2d_layout_are_codewords(lib, oracle, tmp_path):
    """the construction the GPU round trip relies on, by the twin alone: k = 4 polynomials at (256, 4) extended column-wise to 8 rows by the scalar
    transform; the 8 commitments and the 8 proofs of every cell, made row by row through the host producer, are columns of degree < 4 -- from rows
    {0, 3, 4, 7} the twin returns all 8 x 65 points with consistent = 1"""
    from tests.g1_recover_cases import extended_world
    W, columns = extended_world(lib, oracle, tmp_path)
    rows = np.array([7, 0, 4, 3], dtype=np.uint32)
    got, rep = lib.host_g1_recover(rows, np.ascontiguousarray(columns[:, rows]), 8, 4, batch=65)
    assert rep == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, missing=4) and np.array_equal(got, columns)


def test_the_stage_mapping_switch_takes_zero_one_and_two_only(lib):
    from barretenberg_amd import BbGpuError
    for mapping in (2, 1, 0):
        lib.g1_set_stage_mapping(mapping)
    for mapping in (-1, 3):
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.g1_set_stage_mapping(mapping)


def test_host_twins_under_sanitizers(tmp_path):
    """tests/cpp/test_g1_recover_host.cpp: the two twins as a stand-alone program (own main) built with -fsanitize=address,undefined, at (8, 4) and
    (64, 17): transforms there and back, recovery of multiples of the generator, an altered point, refused calls"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_g1_recover_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_g1_recover_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
