"""bbgpu_host_kzg_recover_cells_each (csrc/host_kzg_recover_each.hpp): polynomials of degree < d, each rebuilt from its OWN subset of cells, held to
Lagrange interpolation over Python integers and to the polynomial the cells were made from, bit for bit; to bbgpu_host_kzg_recover_cells when every
polynomial holds the same set; the per-polynomial findings on altered cells; and the argument verdicts of the twin and of the device entry on a machine
without a GPU.  The twin is what the GPU entry is compared with bit for bit (tests/test_gpu_kzg_recover_each.py).  CPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.kzg_recover_cells_cases import ERR_ARG, ERR_SIZE, PAD, call_values, coefficient_buffer, polynomial, present_cells
from tests.kzg_recover_each_cases import NONE, R, each_case, each_values, expected_each, interpolate, memory, spread


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


def recover(lib, n, l, d, cells, values, pad=0, want_values=True):
    """one twin call into a buffer of other values; the padding is untouched afterwards -> (batch, n, 4) coefficients, transforms, report, first_bad"""
    batch, stride = len(cells), n + pad
    buf = coefficient_buffer(batch, stride)
    kept = buf.copy()
    out, vals, rep, first = lib.host_kzg_recover_cells_each(cells, values, n, l, d, stride=stride, want_values=want_values, out=buf)
    assert out is buf
    rows = buf.reshape(batch, stride, 4)
    assert np.array_equal(rows[:, n:], kept.reshape(batch, stride, 4)[:, n:])
    return rows[:, :n], vals, rep, first


def three_sets(n, l, d):
    """all cells but one; a seeded set in between; exactly d / l cells"""
    m = n // l
    return [spread(m, 1, 5), spread(m, (m - d // l) // 2, 6), spread(m, m - d // l, 7)]


@pytest.mark.parametrize("n,l,d", [(32, 4, 8), (64, 4, 16), (64, 1, 16), (32, 1, 5), (64, 4, 14)])
def test_twin_against_interpolation_and_the_original_polynomial(lib, n, l, d):
    sets = three_sets(n, l, d) if d % l == 0 else [spread(n // l, 1, 5), spread(n // l, 9, 6), spread(n // l, n // l - (d + l - 1) // l, 7)]
    cells, ints, polys = each_case(n, l, d, sets)
    assert len({len(c) for c in cells}) == 3 and len(cells[0]) == n // l - 1 and len(cells[2]) == (d + l - 1) // l
    got_c, got_v, rep, first = recover(lib, n, l, d, cells, each_values(ints, l), PAD)
    for b in range(3):
        assert np.array_equal(got_c[b], memory(interpolate(n, l, cells[b], ints[b]))), b
        assert np.array_equal(got_c[b], memory(polys[b][0])), b
        assert np.array_equal(got_v[b], memory(polys[b][1])), b
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=max(len(s) for s in sets))
    assert first.tolist() == [NONE] * 3


@pytest.mark.parametrize("n,l,batch", [(256, 4, 4), (1024, 64, 2)])
def test_same_set_for_every_polynomial_is_the_existing_twin(lib, n, l, batch):
    m, d = n // l, n // 4
    for missing in ([], spread(m, 1), spread(m, m // 3), list(range(0, m, 2)), spread(m, m - d // l)):
        polys = [polynomial(n, d, b) for b in range(batch)]
        same = present_cells(n, l, missing)  # one list for all
        values = call_values([v for _, v in polys], n, l, same)
        for alter in (None, 5):
            if alter is not None:
                if len(same) * l == d:
                    continue
                values = values.copy()
                values[len(same) * l + alter] = memory([0xA17E2ED])[0]  # a value of polynomial 1
            buf = coefficient_buffer(batch, n + PAD)
            want_c, want_v, want_rep = lib.host_kzg_recover_cells(same, values, n, l, d, batch=batch, stride=n + PAD, out=buf.copy())
            per_poly = [values.reshape(batch, len(same), l, 4)[b] for b in range(batch)]
            got_c, got_v, rep, first = lib.host_kzg_recover_cells_each([same] * batch, per_poly, n, l, d, stride=n + PAD, out=buf.copy())
            assert np.array_equal(got_c, want_c) and np.array_equal(got_v, want_v), (len(missing), alter)
            assert {k: rep[k] for k in ("consistent", "first_bad_poly", "first_bad_coeff")} == {k: want_rep[k] for k in ("consistent", "first_bad_poly", "first_bad_coeff")}
            assert rep["max_missing"] == want_rep["missing"] == len(missing)
            assert (rep["consistent"] == 0) == (alter is not None)
            assert first.tolist() == [want_rep["first_bad_coeff"] if (alter is not None and b == 1) else NONE for b in range(batch)]


@pytest.mark.parametrize("n,l,d", [(64, 4, 16), (64, 1, 11)])
def test_one_altered_value_shows_in_its_polynomial_only(lib, n, l, d):
    """polynomial 1 of 3 with redundancy and one value altered: first_bad is [NONE, k, NONE] with the k of the plain-integer interpolation"""
    m = n // l
    sets = [spread(m, 3, 8), spread(m, 5, 9), spread(m, m - (d + l - 1) // l, 10)]
    cells, ints, polys = each_case(n, l, d, sets)
    for spot in (0, len(ints[1]) // 2, len(ints[1]) - 1):
        bent = [list(v) for v in ints]
        bent[1][spot] = (bent[1][spot] + 1 + spot) % R
        want = [list(polys[0][0]), interpolate(n, l, cells[1], bent[1]), list(polys[2][0])]
        want_rep, want_first = expected_each(want, d, cells, l, m)
        assert want_rep["consistent"] == 0 and want_rep["first_bad_poly"] == 1 and d <= want_rep["first_bad_coeff"] < len(cells[1]) * l
        got_c, _, rep, first = recover(lib, n, l, d, cells, each_values(bent, l), PAD)
        assert rep == want_rep and np.array_equal(first, want_first) and first.tolist() == [NONE, want_rep["first_bad_coeff"], NONE], spot
        for b in range(3):
            assert np.array_equal(got_c[b], memory(want[b])), (spot, b)


def test_the_same_alteration_without_redundancy_is_not_seen(lib):
    """count_1 l == d: any values are those of a polynomial of degree < d"""
    n, l, d = 64, 4, 16
    sets = [spread(16, 3, 8), spread(16, 12, 9), spread(16, 5, 10)]
    cells, ints, polys = each_case(n, l, d, sets)
    bent = [list(v) for v in ints]
    bent[1][7] = (bent[1][7] + 1) % R
    got_c, _, rep, first = recover(lib, n, l, d, cells, each_values(bent, l))
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=12) and first.tolist() == [NONE] * 3
    assert np.array_equal(got_c[1], memory(interpolate(n, l, cells[1], bent[1])))


def test_values_out_and_first_bad_out_may_be_left_out(lib):
    from barretenberg_amd.bbgpu import KzgRecoverEachReport, _ptr, u64p
    n, l, d = 16, 4, 8
    cells, ints, polys = each_case(n, l, d, [[1], [0, 3]])
    got_c, got_v, rep, _ = recover(lib, n, l, d, cells, each_values(ints, l), want_values=False)
    assert got_v is None and np.array_equal(got_c[0], memory(polys[0][0])) and np.array_equal(got_c[1], memory(polys[1][0]))
    L, u32p = lib.lib, C.POINTER(C.c_uint32)
    L.bbgpu_host_kzg_recover_cells_each.argtypes = [u32p, u32p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, u64p, C.c_size_t, u64p, u64p,
                                                    C.POINTER(KzgRecoverEachReport)]
    off, flat = np.array([0, 3, 5], dtype=np.uint32), np.concatenate(cells).astype(np.uint32)
    values, out, r = np.concatenate([memory(v) for v in ints]), np.zeros((2 * n, 4), dtype=np.uint64), KzgRecoverEachReport()
    assert L.bbgpu_host_kzg_recover_cells_each(off.ctypes.data_as(u32p), flat.ctypes.data_as(u32p), _ptr(values), n, l, d, 2, _ptr(out), n, None, None, C.byref(r)) == 0
    assert np.array_equal(out.reshape(2, n, 4), got_c) and r.consistent == 1 and r.max_missing == 2


def refusals(n=16, l=4):
    """(kwargs, verdict, text) for every refusal of include/bbgpu.h; everything defaults to a good call at (16, 4), degree bound 8, batch 2"""
    size = [(dict(n=0), ""), (dict(n=1), ""), (dict(n=3), ""), (dict(n=12), ""), (dict(n=1 << 22, l=64), ""), (dict(l=0), ""), (dict(l=3), ""),
            (dict(l=128, n=256), ""), (dict(l=n), ""), (dict(l=2 * n), ""), (dict(d=0), "degree bound"), (dict(d=n + 1), "degree bound"),
            (dict(cells=[[0, 1, 2]] * 0), "batch 0"), (dict(cells=[[0, 1, 2]] * 65), "batch 65"), (dict(stride=n - 1), "stride 15"),
            (dict(n=1 << 20, l=64, d=1, cells=[[0]] * 5), "batch x n"), (dict(n=1 << 17, l=64, d=1, cells=[[0]] * 33), "batch x n"),
            (dict(cells=[[0, 1, 2], []]), "polynomial 1 lists 0 cells"), (dict(cells=[[0, 1, 2], [0, 1, 2, 3, 0]]), "polynomial 1 lists 5 cells"),
            (dict(cells=[[0, 1, 2], [0, 1, 2, 3], [3]], d=5), "polynomial 2 lists 1 cells")]
    arg = [(dict(cells=[[0, 1, 2], [0, 1, 4]]), r"polynomial 1: cell\[5\] = 4 \(position 2 of its list\) is not below"),
           (dict(cells=[[0, 1, 1 << 31], [0, 1]]), r"polynomial 0: cell\[2\] = 2147483648 \(position 2"),
           (dict(cells=[[0, 1, 2], [0, 2, 1, 2]]), r"polynomial 1: cell\[6\] = 2 \(position 3 of its list\) is listed twice"),
           (dict(cells=[[3, 3], [0, 1]]), r"polynomial 0: cell\[1\] = 3 \(position 1 of its list\) is listed twice")]
    return [(k, ERR_SIZE, t) for k, t in size] + [(k, ERR_ARG, t) for k, t in arg]


def refusal_call(kw, n=16, l=4):
    n, l = kw.get("n", n), kw.get("l", l)
    cells = [np.array(c, dtype=np.uint32) for c in kw.get("cells", [[0, 1, 2], [3, 1]])]
    values = [np.zeros((len(c) * max(l, 1), 4), dtype=np.uint64) for c in cells]
    return n, l, kw.get("d", 8), cells, values, kw.get("stride", n)


RAW = lambda u32p, u64p, rep, last: [u32p, u32p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, last, C.c_size_t, u64p, u64p, C.POINTER(rep)]  # noqa: E731


def raw_refusals(call, out_ptr, extra):
    """null pointers and malformed offsets, through the C entry itself: (return value, text pattern)"""
    off, bad0, down = (np.array(a, dtype=np.uint32) for a in ([0, 3, 5], [1, 3, 5], [0, 3, 2]))
    cell, values = np.array([0, 1, 2, 3, 1], dtype=np.uint32), np.zeros((20, 4), dtype=np.uint64)
    from barretenberg_amd.bbgpu import KzgRecoverEachReport, _ptr
    rep = KzgRecoverEachReport()
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    good = [p32(off), p32(cell), _ptr(values), 16, 4, 8, 2, out_ptr, 16, None, None, C.byref(rep)]
    cases = [({0: None}, "null cell offsets"), ({1: None}, "null cell"), ({2: None}, "null cell"), ({7: None}, "null cell"), ({11: None}, "null cell"),
             ({0: p32(bad0)}, r"cell_offsets\[0\] = 1 is not 0"), ({0: p32(down)}, r"polynomial 1: cell_offsets\[2\] = 2 is below cell_offsets\[1\] = 3")]
    for change, text in cases:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        yield call(*args, *extra), text
    yield call(*good, *extra), None


def test_twin_refusals_leave_the_outputs_untouched(lib):
    import re
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import KzgRecoverEachReport, _ptr, u64p
    for kw, verdict, text in refusals():
        n, l, d, cells, values, stride = refusal_call(kw)
        small = coefficient_buffer(1, 32)  # sizes are judged before anything is written: no refused call needs its full output
        kept = small.copy()
        with pytest.raises(BbGpuError, match=verdict + ".*" + text):
            lib.host_kzg_recover_cells_each(cells, values, n, l, d, stride=stride, want_values=False, out=small)
        assert np.array_equal(small, kept), kw
    L = lib.lib
    L.bbgpu_host_kzg_recover_cells_each.argtypes = RAW(C.POINTER(C.c_uint32), u64p, KzgRecoverEachReport, u64p)
    out = coefficient_buffer(2, 16)
    kept = out.copy()
    for rc, text in raw_refusals(L.bbgpu_host_kzg_recover_cells_each, _ptr(out), ()):
        if text is None:
            assert rc == 0 and not np.array_equal(out, kept)  # values_out and first_bad_out may be NULL
        else:
            assert rc == -3 and re.search(text, lib.lib.bbgpu_last_error().decode()) and np.array_equal(out, kept), text


def test_the_device_entry_refuses_its_arguments_before_a_device_is_bound(lib):
    """every refusal again, through bbgpu_kzg_recover_cells_each on a machine without a GPU: nothing is initialised for a call that is refused"""
    import re
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import KzgRecoverEachReport, u64p
    fake = 0x1000  # never dereferenced
    for kw, verdict, text in refusals():
        n, l, d, cells, values, stride = refusal_call(kw)
        with pytest.raises(BbGpuError, match=verdict + ".*" + text):
            lib.kzg_recover_cells_each(cells, values, n, l, d, fake, stride=stride, want_values=False)
    L = lib.lib
    L.bbgpu_kzg_recover_cells_each.argtypes = RAW(C.POINTER(C.c_uint32), u64p, KzgRecoverEachReport, C.c_void_p) + [C.c_void_p]
    for rc, text in raw_refusals(L.bbgpu_kzg_recover_cells_each, fake, (None,)):
        if text is not None:
            assert rc == -3 and re.search(text, lib.lib.bbgpu_last_error().decode()), text


def test_host_twin_under_sanitizers(tmp_path):
    """tests/cpp/test_kzg_recover_each_host.cpp: the twin as a stand-alone program (own main) built with -fsanitize=address,undefined: (16, 4) and (64, 1),
    batch 3 with different sets and padding, against the polynomials the cells were made from; an altered value; refused calls"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kzg_recover_each_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_kzg_recover_each_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
