"""bbgpu_host_kzg_recover_cells (csrc/host_kzg_recover_cells.hpp): polynomials of degree < d rebuilt from a subset of their cells through the vanishing
polynomial of the missing ones, held to the polynomial the cells were made from, bit for bit, and at n <= 64 to Lagrange interpolation over Python
integers (tests/kzg_recover_cells_cases.py) -- the twin the GPU entry is compared with bit for bit (tests/test_gpu_kzg_recover_cells.py) -- the consistency
verdict on altered cells, and the argument verdicts of the twin and of the device entry on a machine without a GPU.  CPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.kzg_recover_cells_cases import (ALL_ONES, ERR_ARG, ERR_SIZE, PAD, R, add_modulus, call_values, coefficient_buffer, expected_report, from_int,
                                           interpolate, listed_values, memory, missing_sets, plain, polynomial, present_cells)

SIZES = [(4, 2), (8, 1), (16, 4), (64, 16), (256, 4), (8192, 64)]


def degree_bounds(n, l):
    return sorted({d for d in (1, l - 1, l, n // 2, n // 2 + 1, n) if 1 <= d <= n})


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


def recover(lib, n, l, d, cells, values, batch, pad=0, want_values=True):
    """one twin call into a buffer of other values; the inputs are unchanged and the padding untouched afterwards -> (batch, n, 4) coefficients, the
    transforms, the report"""
    stride = n + pad
    buf = coefficient_buffer(batch, stride)
    kept, cells_kept, values_kept = buf.copy(), cells.copy(), values.copy()
    out, vals, rep = lib.host_kzg_recover_cells(cells, values, n, l, d, batch=batch, stride=stride, want_values=want_values, out=buf)
    assert out is buf and np.array_equal(cells, cells_kept) and np.array_equal(values, values_kept)
    rows = buf.reshape(batch, stride, 4)
    assert np.array_equal(rows[:, n:], kept.reshape(batch, stride, 4)[:, n:])
    return rows[:, :n], vals, rep


@pytest.mark.parametrize("n,l", SIZES)
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, PAD)])
def test_twin_against_the_original_polynomial(lib, n, l, batch, pad):
    """every degree bound and every kind of missing set that fits it, cells listed in shuffled order"""
    for d in degree_bounds(n, l):
        polys = [polynomial(n, d, b) for b in range(batch)]
        want_c = np.stack([memory(c) for c, _ in polys])
        want_v = np.stack([memory(v) for _, v in polys])
        for name, missing in missing_sets(n, l, d).items():
            cells = present_cells(n, l, missing)
            got_c, got_v, rep = recover(lib, n, l, d, cells, call_values([v for _, v in polys], n, l, cells), batch, pad)
            assert np.array_equal(got_c, want_c), (d, name)
            assert np.array_equal(got_v, want_v), (d, name)
            assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, missing=len(missing)), (d, name)


def test_values_out_may_be_left_out(lib):
    n, l, d = 16, 4, 8
    (c, v), cells = polynomial(n, d), present_cells(n, l, [1, 2])
    got_c, got_v, _ = recover(lib, n, l, d, cells, call_values([v], n, l, cells), 1, want_values=False)
    assert got_v is None and np.array_equal(got_c[0], memory(c))


@pytest.mark.parametrize("n,l", [(4, 2), (8, 1), (16, 4), (64, 16), (64, 1)])
def test_twin_against_interpolation(lib, n, l):
    """n <= 64: the twin's coefficients are those of the interpolating polynomial through the listed points, for honest cells and for cells with one value
    altered (where the original polynomial is no longer the answer)"""
    for d in degree_bounds(n, l):
        _, v = polynomial(n, d)
        for name, missing in missing_sets(n, l, d).items():
            cells = present_cells(n, l, missing)
            vals = listed_values(v, n, l, cells)
            for alter in (False, True):
                if alter:
                    vals[len(vals) // 2] = (vals[len(vals) // 2] + 1) % R
                want = interpolate(n, l, cells, vals)
                got_c, _, rep = recover(lib, n, l, d, cells, memory(vals), 1)
                assert np.array_equal(got_c[0], memory(want)), (d, name, alter)
                assert rep == expected_report([want], d, len(cells) * l, len(missing)), (d, name, alter)


@pytest.mark.parametrize("n,l,d,missing", [(16, 4, 5, [0, 3]), (64, 16, 17, [2]), (64, 1, 11, list(range(20, 50)))])
def test_one_altered_value_among_redundant_cells_always_shows(lib, n, l, d, missing):
    """batch 3, count l > d, one value of polynomial 1 altered: consistent = 0, the first bad polynomial and coefficient are what the plain-integer recovery
    gives, and the other two polynomials are still exact"""
    polys, cells = [polynomial(n, d, b) for b in range(3)], present_cells(n, l, missing)
    vals = [listed_values(v, n, l, cells) for _, v in polys]
    for spot in range(len(vals[1])):  # EVERY position: the verdict is exact, not probabilistic
        bent = [list(v) for v in vals]
        bent[1][spot] = (bent[1][spot] + 1 + spot) % R
        want = [list(polys[0][0]), interpolate(n, l, cells, bent[1]), list(polys[2][0])]
        rep_want = expected_report(want, d, len(cells) * l, len(missing))
        assert rep_want["consistent"] == 0 and rep_want["first_bad_poly"] == 1 and d <= rep_want["first_bad_coeff"] < len(cells) * l
        got_c, _, rep = recover(lib, n, l, d, cells, memory([x for v in bent for x in v]), 3, PAD)
        assert rep == rep_want, spot
        for b in range(3):
            assert np.array_equal(got_c[b], memory(want[b])), (spot, b)


def test_an_altered_value_without_redundancy_is_not_seen(lib):
    """count l == d: any values are the values of a polynomial of degree < d, and the report says consistent (include/bbgpu.h says so too)"""
    n, l, d = 16, 4, 8
    (_, v), cells = polynomial(n, d), present_cells(n, l, [0, 2])
    vals = listed_values(v, n, l, cells)
    vals[3] = (vals[3] + 1) % R
    got_c, _, rep = recover(lib, n, l, d, cells, memory(vals), 1)
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, missing=2)
    assert np.array_equal(got_c[0], memory(interpolate(n, l, cells, vals)))


def test_values_given_as_other_representatives(lib):
    """v + r in every other row; and the constant polynomial whose value is given as 2^256 - 1, which the library reduces"""
    n, l, d = 64, 16, 20
    (c, v), cells = polynomial(n, d), present_cells(n, l, [1])
    values = call_values([v], n, l, cells)
    got_c, got_v, rep = recover(lib, n, l, d, cells, add_modulus(values, range(0, values.shape[0], 2)), 1)
    assert np.array_equal(got_c[0], memory(c)) and np.array_equal(got_v[0], memory(v)) and rep["consistent"] == 1
    ones = np.tile(from_int(ALL_ONES), (len(cells) * l, 1))
    got_c, got_v, rep = recover(lib, n, l, 1, cells, ones, 1)
    const = plain(ones[:1])[0]
    assert np.array_equal(got_c[0], memory([const] + [0] * (n - 1))) and np.array_equal(got_v[0], memory([const] * n)) and rep["consistent"] == 1


def refusals(n=16, l=4):
    """(kwargs, verdict) for every refusal of include/bbgpu.h; n, coset, d, batch, stride and the cell list default to a good call at (16, 4)"""
    m = n // l
    size = [dict(n=0), dict(n=1), dict(n=3), dict(n=12), dict(n=1 << 22, l=64), dict(l=0), dict(l=3), dict(l=128, n=256), dict(l=n), dict(l=2 * n),
            dict(n=1 << 17, l=1), dict(n=1 << 21, l=16),  # m above 2^16
            dict(d=0), dict(d=n + 1), dict(cells=[0, 1], d=9), dict(cells=[0, 1, 2, 3, 0], d=1),  # too few cells; more than m
            dict(batch=0), dict(batch=-1), dict(batch=65), dict(stride=n - 1), dict(n=1 << 20, l=64, d=1, batch=5), dict(n=1 << 17, l=64, d=1, batch=33)]
    arg = [dict(cells=[0, 1, m]), dict(cells=[0, 1, 1 << 31]), dict(cells=[0, 2, 1, 2]), dict(cells=[3, 3])]
    return [(k, ERR_SIZE) for k in size] + [(k, ERR_ARG) for k in arg]


def refusal_call(kw, n=16, l=4):
    n, l = kw.get("n", n), kw.get("l", l)
    cells = np.array(kw.get("cells", [0, 1, 2]), dtype=np.uint32)
    batch = kw.get("batch", 1)
    values = np.zeros((max(batch, 1) * len(cells) * max(l, 1), 4), dtype=np.uint64)
    return n, l, kw.get("d", 8), cells, values, batch, kw.get("stride", n)


def test_twin_refusals_leave_the_outputs_untouched(lib):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import KzgRecoverReport, _ptr, u64p
    for kw, verdict in refusals():
        n, l, d, cells, values, batch, stride = refusal_call(kw)
        small = coefficient_buffer(1, 32)  # sizes are judged before anything is written: no refused call needs its full output
        kept = small.copy()
        with pytest.raises(BbGpuError, match=verdict):
            lib.host_kzg_recover_cells(cells, values, n, l, d, batch=batch, stride=stride, want_values=False, out=small)
        assert np.array_equal(small, kept), kw
    with pytest.raises(BbGpuError, match=ERR_ARG + ".*cell\\[2\\] = 1 is listed twice"):  # the first offender is named
        lib.host_kzg_recover_cells(np.array([0, 1, 1, 9], dtype=np.uint32), np.zeros((16, 4), dtype=np.uint64), 16, 4, 8)
    with pytest.raises(BbGpuError, match=ERR_ARG + ".*cell\\[1\\] = 4 is not below"):
        lib.host_kzg_recover_cells(np.array([0, 4, 4], dtype=np.uint32), np.zeros((12, 4), dtype=np.uint64), 16, 4, 8)
    L = lib.lib
    u32p = C.POINTER(C.c_uint32)
    L.bbgpu_host_kzg_recover_cells.argtypes = [u32p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, u64p, C.c_size_t, u64p,
                                               C.POINTER(KzgRecoverReport)]
    cells, values, out, rep = np.array([0, 1, 2], dtype=np.uint32), np.zeros((12, 4), dtype=np.uint64), coefficient_buffer(1, 16), KzgRecoverReport()
    cp, kept = cells.ctypes.data_as(u32p), out.copy()
    for args in ((None, 3, _ptr(values), 16, 4, 8, 1, _ptr(out), 16, None, C.byref(rep)), (cp, 3, None, 16, 4, 8, 1, _ptr(out), 16, None, C.byref(rep)),
                 (cp, 3, _ptr(values), 16, 4, 8, 1, None, 16, None, C.byref(rep)), (cp, 3, _ptr(values), 16, 4, 8, 1, _ptr(out), 16, None, None)):
        assert L.bbgpu_host_kzg_recover_cells(*args) == -3
    assert np.array_equal(out, kept)
    assert L.bbgpu_host_kzg_recover_cells(cp, 3, _ptr(values), 16, 4, 8, 1, _ptr(out), 16, None, C.byref(rep)) == 0  # values_out may be NULL


def test_the_device_entry_refuses_its_arguments_before_a_device_is_bound(lib):
    """every refusal again, through bbgpu_kzg_recover_cells on a machine without a GPU: nothing is initialised for a call that is refused"""
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import KzgRecoverReport, _ptr, u64p
    fake = 0x1000  # never dereferenced
    for kw, verdict in refusals():
        n, l, d, cells, values, batch, stride = refusal_call(kw)
        with pytest.raises(BbGpuError, match=verdict):
            lib.kzg_recover_cells(cells, values, n, l, d, fake, batch=batch, stride=stride, want_values=False)
    L = lib.lib
    u32p = C.POINTER(C.c_uint32)
    L.bbgpu_kzg_recover_cells.argtypes = [u32p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, u64p,
                                          C.POINTER(KzgRecoverReport), C.c_void_p]
    cells, values, rep = np.array([0, 1, 2], dtype=np.uint32), np.zeros((12, 4), dtype=np.uint64), KzgRecoverReport()
    cp = cells.ctypes.data_as(u32p)
    for args in ((None, 3, _ptr(values), 16, 4, 8, 1, fake, 16, None, C.byref(rep), None), (cp, 3, None, 16, 4, 8, 1, fake, 16, None, C.byref(rep), None),
                 (cp, 3, _ptr(values), 16, 4, 8, 1, None, 16, None, C.byref(rep), None), (cp, 3, _ptr(values), 16, 4, 8, 1, fake, 16, None, None, None)):
        assert L.bbgpu_kzg_recover_cells(*args) == -3


def test_host_twin_under_sanitizers(tmp_path):
    """tests/cpp/test_kzg_recover_cells_host.cpp: the twin as a stand-alone program (own main) built with -fsanitize=address,undefined: (8, 1), (16, 4) and
    (256, 64), batch 1 and 3 with padding, against the polynomial the cells were made from; altered values; refused calls"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kzg_recover_cells_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_kzg_recover_cells_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
