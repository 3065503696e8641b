"""bbgpu_host_fr_ntt_columns and bbgpu_host_fr_recover_columns (csrc/host_fr_columns.hpp): the transform and the erasure decoder down the columns of a
row-major matrix, held to statements that share no code with them -- Lagrange interpolation over Python integers at rows <= 16, bbgpu_host_ntt column by
column, and bbgpu_host_kzg_recover_cells_each at coset 1 on the transposed matrix bit for bit.  Then what a call may touch (present rows and padding stay
bit for bit, also for non-canonical inputs and in an inconsistent column), the verdict, every refusal of include/bbgpu.h through the twin and through the
device entry on a machine without a GPU, and the linearity across rows.  The twin is what the GPU entry is compared with bit for bit
(tests/test_gpu_fr_columns.py).  CPU tests."""
import ctypes as C
import re

import numpy as np
import pytest

from tests.fr_columns_cases import (ERR_ARG, ERR_SIZE, JUNK, NONE, PAD, R, SENTINEL, add_modulus_where_it_fits, alter, clean_report, codeword_ints,
                                    erase, expected_first_bad, lagrange_column, matrix_memory, memory, missing_mask, missing_of, plain, report_of, row_sets,
                                    transform)

SMALL = [(2, 1, 3, (1, 0, 1)), (4, 2, 5, (2,)), (8, 4, 7, (4, 0, 3)), (16, 5, 6, (11, 1, 7, 0, 11, 3))]  # (rows, d, width, missing per set)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


def case(rows, d, width, mus, seed=0):
    ints = codeword_ints(rows, width, d, seed)
    sets_rows = row_sets(rows, mus)
    stride = width + PAD
    full = matrix_memory(ints, stride)
    return ints, sets_rows, stride, full, erase(full, rows, width, stride, sets_rows)


def ints_of(mem, rows, width, stride):
    m = mem.reshape(rows, stride, 4)
    return [plain(m[r, :width]) for r in range(rows)]


@pytest.mark.parametrize("rows,d,width,mus", SMALL)
def test_twin_equals_lagrange_interpolation(lib, rows, d, width, mus):
    ints, sets_rows, stride, full, held = case(rows, d, width, mus)
    rep, first_bad = lib.host_fr_recover_columns(sets_rows, held, rows, width, d, stride=stride)
    assert rep == clean_report(rows, sets_rows) and all(int(v) == NONE for v in first_bad)
    assert np.array_equal(held, full)  # canonical, bit for bit: the codewords one started from, padding included
    got = ints_of(held, rows, width, stride)
    for j in range(width):
        _, values = lagrange_column(rows, sets_rows[j % len(sets_rows)], [ints[r][j] for r in range(rows)])
        assert [got[r][j] for r in range(rows)] == values, j


@pytest.mark.parametrize("rows,d,width,mus", SMALL)
def test_altered_values_recover_to_the_interpolation_and_are_found_where_the_definition_finds_them(lib, rows, d, width, mus):
    ints, sets_rows, stride, full, held = case(rows, d, width, mus)
    for j in range(width):  # one altered present element in every column
        r = int(sets_rows[j % len(sets_rows)][0])
        alter(held, stride, r, j)
        ints[r][j] = (ints[r][j] + 1) % R
    before = held.copy()
    rep, first_bad = lib.host_fr_recover_columns(sets_rows, held, rows, width, d, stride=stride)
    want_bad = expected_first_bad(rows, d, sets_rows, ints)
    assert [int(v) for v in first_bad] == want_bad and rep == report_of(want_bad, rows, sets_rows)
    gone = missing_mask(rows, width, sets_rows)
    keep = np.ones((rows, stride), dtype=bool)
    keep[:, :width] = ~gone
    assert np.array_equal(held.reshape(rows, stride, 4)[keep], before.reshape(rows, stride, 4)[keep])  # present rows and padding, in inconsistent columns too
    got = ints_of(held, rows, width, stride)
    for j in range(width):
        present = sets_rows[j % len(sets_rows)]
        _, values = lagrange_column(rows, present, [ints[r][j] for r in range(rows)])
        for r in missing_of(rows, present):
            assert got[r][j] == values[r], (j, r)
    # vacuous where count_s == d: such a column is never named
    for j in range(width):
        if len(sets_rows[j % len(sets_rows)]) == d:
            assert int(first_bad[j]) == NONE


@pytest.mark.parametrize("rows,width", [(2, 3), (8, 5), (16, 4), (64, 3), (2048, 2)])
@pytest.mark.parametrize("kind", ["fft", "ifft"])
def test_ntt_columns_equals_host_ntt_column_by_column(lib, rows, width, kind):
    rng = np.random.default_rng([rows, width])
    stride = width + PAD
    mem = matrix_memory([[int.from_bytes(rng.bytes(32), "little") % R for _ in range(width)] for _ in range(rows)], stride)
    mem[:width] = add_modulus_where_it_fits(mem[:width])[0]  # non-canonical inputs in row 0
    m = mem.reshape(rows, stride, 4)
    first = plain(m[:, 0])
    want = np.stack([lib.host_ntt(np.ascontiguousarray(m[:, j]), kind) for j in range(width)], axis=1)
    lib.host_fr_ntt_columns(mem, rows, width, kind, stride=stride)
    assert np.array_equal(m[:, :width], want) and np.all(m[:, width:] == np.uint64(SENTINEL))
    if rows <= 16:  # against the definition over Python integers; the inverse with its rows^-1: the forward transform brings the column back
        assert (plain(m[:, 0]) == transform(first, rows)) if kind == "fft" else (transform(plain(m[:, 0]), rows) == first)


def each_on_the_transpose(lib, held, rows, width, stride, sets_rows, d):
    """bbgpu_host_kzg_recover_cells_each at coset 1, fed every column with its own set"""
    m = held.reshape(rows, stride, 4)
    cells = [sets_rows[j % len(sets_rows)] for j in range(width)]
    values = [np.ascontiguousarray(m[np.asarray(c, dtype=np.int64), j]) for j, c in enumerate(cells)]
    _, vals, rep, first_bad = lib.host_kzg_recover_cells_each(cells, values, rows, 1, d)
    return vals, rep, first_bad


@pytest.mark.parametrize("rows,d,width,mus", SMALL + [(64, 17, 64, (30, 0, 47, 1, 5)), (512, 100, 9, (300, 5, 412))])
@pytest.mark.parametrize("altered", [False, True])
def test_twin_equals_the_row_decoder_on_the_transpose_bit_for_bit(lib, rows, d, width, mus, altered):
    from tests.fr_columns_cases import codeword_memory
    sets_rows = row_sets(rows, mus)
    stride = width + PAD
    full = matrix_memory(codeword_ints(rows, width, d), stride) if rows <= 64 else codeword_memory(lib, rows, width, d, stride)
    held = erase(full, rows, width, stride, sets_rows)
    if altered:
        j = width - 1
        alter(held, stride, int(sets_rows[j % len(sets_rows)][-1]), j)
    vals, each_rep, each_bad = each_on_the_transpose(lib, held, rows, width, stride, sets_rows, d)
    rep, first_bad = lib.host_fr_recover_columns(sets_rows, held, rows, width, d, stride=stride)
    assert rep == dict(consistent=each_rep["consistent"], first_bad_column=each_rep["first_bad_poly"], first_bad_coeff=each_rep["first_bad_coeff"],
                       max_missing=each_rep["max_missing"])
    assert [int(v) for v in first_bad] == [NONE if int(v) == (1 << 64) - 1 else int(v) for v in each_bad]
    gone = missing_mask(rows, width, sets_rows)
    assert np.array_equal(held.reshape(rows, stride, 4)[:, :width][gone], vals.transpose(1, 0, 2)[gone])
    if not altered:
        assert np.array_equal(held, full) and rep["consistent"] == 1
    elif len(sets_rows[(width - 1) % len(sets_rows)]) > d:
        assert rep["consistent"] == 0 and rep["first_bad_column"] == width - 1


def test_non_canonical_inputs_give_the_same_outputs_and_stay_as_they_are(lib):
    rows, d, width, mus = 8, 3, 7, (4, 0, 5)
    ints, sets_rows, stride, full, held = case(rows, d, width, mus)
    other, changed = add_modulus_where_it_fits(held)  # JUNK and the sentinel do not fit
    assert changed > rows * width // 4
    before = other.copy()
    rep, first_bad = lib.host_fr_recover_columns(sets_rows, other, rows, width, d, stride=stride)
    assert rep == clean_report(rows, sets_rows)
    gone = np.zeros((rows, stride), dtype=bool)
    gone[:, :width] = missing_mask(rows, width, sets_rows)
    o, f, b = other.reshape(rows, stride, 4), full.reshape(rows, stride, 4), before.reshape(rows, stride, 4)
    assert np.array_equal(o[gone], f[gone]) and np.array_equal(o[~gone], b[~gone])


def test_the_report_names_the_smallest_column(lib):
    rows, d, width, mus = 16, 5, 9, (3, 8)
    ints, sets_rows, stride, full, held = case(rows, d, width, mus)
    for j in (6, 2):
        alter(held, stride, int(sets_rows[j % 2][1]), j)
    rep, first_bad = lib.host_fr_recover_columns(sets_rows, held, rows, width, d, stride=stride)
    assert [int(v) != NONE for v in first_bad] == [j in (2, 6) for j in range(width)]
    assert rep["consistent"] == 0 and rep["first_bad_column"] == 2 and rep["first_bad_coeff"] == int(first_bad[2]) and d <= rep["first_bad_coeff"] < 16 - 3
    rep2, none = lib.host_fr_recover_columns(sets_rows, held.copy(), rows, width, d, stride=stride, want_first_bad=False)  # first_bad_out may be NULL
    assert none is None and rep2 == rep


def test_linearity_across_rows(lib):
    """sets = 1, the rows hold COEFFICIENTS: recovering and then transforming each row equals transforming each row and then recovering"""
    rows, d, width = 8, 4, 16
    ints = codeword_ints(rows, width, d, seed=3)  # row r: 16 coefficients of polynomial r; the 8 polynomials are a codeword in every coefficient
    sets_rows = row_sets(rows, (4,))
    full = matrix_memory(ints, width)
    a = erase(full, rows, width, width, sets_rows)
    b = a.copy()
    rep_a, _ = lib.host_fr_recover_columns(sets_rows, a, rows, width, d)
    for r in range(rows):
        a[r * width:(r + 1) * width] = lib.host_ntt(np.ascontiguousarray(a[r * width:(r + 1) * width]), "fft")
    for r in sets_rows[0]:  # the rows one holds
        r = int(r)
        b[r * width:(r + 1) * width] = lib.host_ntt(np.ascontiguousarray(b[r * width:(r + 1) * width]), "fft")
    rep_b, _ = lib.host_fr_recover_columns(sets_rows, b, rows, width, d)
    assert rep_a == rep_b == clean_report(rows, sets_rows) and np.array_equal(a, b)
    assert not np.any(a == np.uint64(JUNK))


# ---- the refusals of include/bbgpu.h: through the twin, and through the device entry before a device is bound ------------------------------------------
def refusals():
    rows, width = 8, 6
    ok = dict(row_sets=[np.arange(6, dtype=np.uint32), np.array([7, 1, 2, 3], dtype=np.uint32)], rows=rows, width=width, stride=width + 1, d=4, offsets=None,
              sets=None)
    out = []

    def add(name, code, text, **kw):
        out.append(pytest.param(dict(ok, **kw), code, text, id=name))
    add("rows-not-a-power-of-two", ERR_SIZE, "rows = 6", rows=6)
    add("rows-below-2", ERR_SIZE, "rows = 1", rows=1)
    add("rows-above-the-cap", ERR_SIZE, "rows = 4096", rows=4096)
    add("width-0", ERR_SIZE, "width 0", width=0)
    add("stride-below-width", ERR_SIZE, "stride 5", stride=5)
    add("rows-x-width-above-2^28", ERR_SIZE, "2^28", width=(1 << 25) + 1, stride=(1 << 25) + 1)
    add("sets-0", ERR_SIZE, "sets = 0", row_sets=[], offsets=np.zeros(1, dtype=np.uint32), sets=0)
    add("sets-above-width", ERR_SIZE, "sets = 7", sets=7, offsets=np.zeros(8, dtype=np.uint32))
    add("sets-x-rows-above-2^20", ERR_SIZE, "2^20", width=1 << 18, stride=1 << 18, sets=(1 << 17) + 1, offsets=np.zeros((1 << 17) + 2, dtype=np.uint32))
    add("degree-bound-0", ERR_SIZE, "degree bound 0", d=0)
    add("degree-bound-above-rows", ERR_SIZE, "degree bound 9", d=9)
    add("count-below-the-degree-bound", ERR_SIZE, "set 1 lists 4 rows", d=5)
    add("count-above-rows", ERR_SIZE, "set 0 lists 9 rows", row_sets=[np.arange(9, dtype=np.uint32), np.arange(4, dtype=np.uint32)])
    add("offsets-do-not-start-at-0", ERR_ARG, "set_offsets[0] = 1", offsets=np.array([1, 6, 10], dtype=np.uint32))
    add("offsets-decrease", ERR_ARG, "set 1: set_offsets[2] = 5 is below set_offsets[1] = 6", offsets=np.array([0, 6, 5], dtype=np.uint32))
    add("row-not-below-rows", ERR_ARG, "set 1: row[7] = 8 (position 1 of its list)", row_sets=[np.arange(6, dtype=np.uint32), np.array([7, 8, 2, 3], dtype=np.uint32)])
    add("row-listed-twice", ERR_ARG, "set 1: row[9] = 1 (position 3 of its list) is listed twice",
        row_sets=[np.arange(6, dtype=np.uint32), np.array([7, 1, 2, 1], dtype=np.uint32)])
    return out


@pytest.mark.parametrize("args,code,text", refusals())
@pytest.mark.parametrize("entry", ["host", "device"])
def test_refusals_leave_the_outputs_alone_and_name_the_offender(lib, entry, args, code, text):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import FrRecoverColumnsReport
    mem = np.full((8 * 7, 4), 0x1234, dtype=np.uint64)  # never reached by a refused call, whatever sizes it names
    first_bad = np.full(8, 0x77, dtype=np.uint32)
    rep = FrRecoverColumnsReport(9, 9, 9, 9)
    with pytest.raises(BbGpuError, match=re.escape(code)) as err:
        if entry == "host":
            lib.host_fr_recover_columns(args["row_sets"], mem, args["rows"], args["width"], args["d"], stride=args["stride"], offsets=args["offsets"],
                                        sets=args["sets"], first_bad=first_bad, report=rep)
        else:  # the device entry refuses before a device is bound: no GPU is needed, and the pointer is never followed
            lib.fr_recover_columns_device(args["row_sets"], mem.ctypes.data, args["rows"], args["width"], args["d"], stride=args["stride"],
                                          offsets=args["offsets"], sets=args["sets"])
    assert text in str(err.value), str(err.value)
    assert np.all(mem == np.uint64(0x1234)) and np.all(first_bad == 0x77) and rep.as_dict() == dict(consistent=9, first_bad_column=9, first_bad_coeff=9, max_missing=9)


def test_null_pointers_and_kinds_are_refused(lib):
    from barretenberg_amd import BbGpuError
    sets_rows = [np.arange(6, dtype=np.uint32)]
    mem = np.zeros((8 * 6, 4), dtype=np.uint64)
    with pytest.raises(BbGpuError, match=re.escape(ERR_ARG)):
        lib.host_fr_recover_columns(sets_rows, None, 8, 6, 4)
    with pytest.raises(BbGpuError, match=re.escape(ERR_ARG)):
        lib.fr_recover_columns_device(sets_rows, None, 8, 6, 4)
    u32p = C.POINTER(C.c_uint32)
    off = np.array([0, 6], dtype=np.uint32)
    f = lib.lib.bbgpu_host_fr_recover_columns
    f.argtypes = [u32p, u32p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, u32p, C.c_void_p]
    assert f(off.ctypes.data_as(u32p), sets_rows[0].ctypes.data_as(u32p), 1, mem.ctypes.data, 8, 6, 6, 4, None, None) == -3  # null report
    assert f(None, sets_rows[0].ctypes.data_as(u32p), 1, mem.ctypes.data, 8, 6, 6, 4, None, None) == -3  # null offsets
    assert f(off.ctypes.data_as(u32p), None, 1, mem.ctypes.data, 8, 6, 6, 4, None, None) == -3  # null rows
    for bad_kind in (2, 3, 4, -1, 7):  # the coset and constant kinds, and no kind at all
        with pytest.raises(BbGpuError, match=re.escape(ERR_ARG)) as err:
            lib.host_fr_ntt_columns(mem, 8, 6, bad_kind)
        assert "kind %d" % bad_kind in str(err.value)
        with pytest.raises(BbGpuError, match=re.escape(ERR_ARG)):
            lib.fr_ntt_columns_device(mem.ctypes.data, 8, 6, bad_kind)
    with pytest.raises(BbGpuError, match=re.escape(ERR_ARG)):
        lib.host_fr_ntt_columns(None, 8, 6, "fft")
    for kw in (dict(rows=6), dict(rows=4096), dict(width=0), dict(stride=5), dict(width=(1 << 25) + 1, stride=(1 << 25) + 1)):
        a = dict(dict(rows=8, width=6, stride=6), **kw)
        with pytest.raises(BbGpuError, match=re.escape(ERR_SIZE)):
            lib.host_fr_ntt_columns(mem, a["rows"], a["width"], "fft", stride=a["stride"])
        with pytest.raises(BbGpuError, match=re.escape(ERR_SIZE)):
            lib.fr_ntt_columns_device(mem.ctypes.data, a["rows"], a["width"], "fft", stride=a["stride"])
    assert not mem.any()
