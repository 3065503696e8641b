"""bbgpu_host_srs_lagrange_check (csrc/host_srs_lagrange_check.hpp): is this table the Lagrange form of that string, on the host -- the definition the GPU
entry's reports are compared with field for field (tests/test_gpu_srs_lagrange_check.py).  CPU tests, no GPU.  The Lagrange tables come from
bbgpu_host_srs_lagrange, itself held to the definition by tests/test_srs_lagrange_host.py."""
import numpy as np
import pytest

from oracle.pyoracle import FQ, aligned_copy
from tests.srs_check_cases import SEED
from tests.srs_lagrange_cases import ERR_ARG, ERR_SIZE, NONE, honest_table, secret_x, tampered, unrelated_points

SIZES = [64, 1024]


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def tables(lib, oracle):
    """per size and kind: (the string, its Lagrange table); made once, never written to"""
    big = honest_table(oracle, secret_x(oracle), max(SIZES))
    out = {}
    for n in SIZES:
        for kind, t in (("honest", aligned_copy(big[:2 * n])), ("unrelated", oracle.point_table(unrelated_points(oracle, n)))):
            out[(n, kind)] = (t, lib.host_srs_lagrange(t, n)[0])
    return out


def verdict(rep):
    return (rep.n, rep.bad_points, rep.first_bad_point, rep.basis_checked, rep.basis_ok, rep.first_bad_row)


def replaced(oracle, lagrange, k, by):
    """row k replaced by row `by` (another point of the curve), its endomorphism entry with it"""
    t = aligned_copy(lagrange)
    t[2 * k:2 * k + 2] = lagrange[2 * by:2 * by + 2]
    return t


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["honest", "unrelated"])
def test_a_converted_table_passes(lib, tables, n, kind):
    mono, lag = tables[(n, kind)]
    for locate in (False, True):
        rep = lib.host_srs_lagrange_check(lag, mono, seed=SEED, locate=locate)
        assert verdict(rep) == (n, 0, NONE, 1, 1, NONE) and rep.ok
        assert np.array_equal(np.array(rep.a), np.array(rep.b)) and list(rep.seed) == [int(v) for v in SEED]


@pytest.mark.parametrize("n", SIZES)
def test_a_wrong_row_is_located(lib, oracle, tables, n):
    mono, lag = tables[(n, "honest")]
    for k in (0, 1, n // 2, n - 1):
        t = replaced(oracle, lag, k, (k + 7) % n)
        rep = lib.host_srs_lagrange_check(t, mono, seed=SEED, locate=True)
        assert verdict(rep) == (n, 0, NONE, 1, 0, k) and not rep.ok
        rep = lib.host_srs_lagrange_check(t, mono, seed=SEED)  # without LOCATE: the verdict alone
        assert verdict(rep) == (n, 0, NONE, 1, 0, NONE)
    t = aligned_copy(lag)  # two rows exchanged: the smaller index
    i, j = n // 4 + 1, n // 2 + 3
    t[[2 * i, 2 * i + 1, 2 * j, 2 * j + 1]] = t[[2 * j, 2 * j + 1, 2 * i, 2 * i + 1]]
    assert verdict(lib.host_srs_lagrange_check(t, mono, seed=SEED, locate=True)) == (n, 0, NONE, 1, 0, i)
    t = aligned_copy(lag)  # a negated row is still on the curve
    t[2 * 5, 4:8] = oracle.neg(FQ, t[2 * 5, 4:8])
    assert verdict(lib.host_srs_lagrange_check(t, mono, seed=SEED, locate=True)) == (n, 0, NONE, 1, 0, 5)


def test_the_string_matters(lib, tables):
    """the Lagrange table of one string against another string"""
    n = 64
    rep = lib.host_srs_lagrange_check(tables[(n, "honest")][1], tables[(n, "unrelated")][0], seed=SEED, locate=True)
    assert verdict(rep) == (n, 0, NONE, 1, 0, 0)
    rep = lib.host_srs_lagrange_check(tables[(n, "honest")][0], tables[(n, "honest")][0], seed=SEED)  # a monomial table is not its own Lagrange form
    assert verdict(rep)[3:5] == (1, 0)


def test_an_off_curve_row_stops_the_check(lib, tables):
    n = 64
    mono, lag = tables[(n, "honest")]
    rep = lib.host_srs_lagrange_check(tampered(tampered(lag, 40), 9), mono, seed=SEED, locate=True)
    assert verdict(rep) == (n, 2, 9, 0, 0, NONE) and not rep.ok
    assert rep.a[7] == 1 << 63 and rep.b[7] == 1 << 63  # no sums taken
    rep = lib.host_srs_lagrange_check(lag, tampered(mono, 3), seed=SEED)  # the string's own rows are bbgpu_srs_check's question: only a different sum
    assert verdict(rep)[:5] == (n, 0, NONE, 1, 0)


def test_seeds(lib, tables):
    n = 64
    mono, lag = tables[(n, "honest")]
    a = lib.host_srs_lagrange_check(lag, mono, seed=SEED).as_dict()
    assert a == lib.host_srs_lagrange_check(lag, mono, seed=SEED).as_dict()  # reproducible
    other = lib.host_srs_lagrange_check(lag, mono, seed=SEED + np.uint64(1)).as_dict()
    assert other["a"] != a["a"] and other["ok"]
    drawn = [lib.host_srs_lagrange_check(lag, mono).as_dict() for _ in range(2)]  # NULL: drawn from the operating system, and reported
    assert all(d["ok"] and any(d["seed"]) for d in drawn) and drawn[0]["seed"] != drawn[1]["seed"]
    assert lib.host_srs_lagrange_check(lag, mono, seed=np.array(drawn[0]["seed"], dtype=np.uint64)).as_dict() == drawn[0]


def test_a_prefix_of_larger_tables(lib, tables):
    """n below the tables' size: rows [0, n) of both -- the first 64 rows of the 1024-row Lagrange table are no Lagrange form of 64 rows"""
    mono, lag = tables[(1024, "honest")]
    assert verdict(lib.host_srs_lagrange_check(lag, mono, n=64, seed=SEED))[3:5] == (1, 0)


def test_arguments(lib, tables):
    from barretenberg_amd import BbGpuError
    import ctypes as C
    from barretenberg_amd.bbgpu import SrsLagrangeCheckReport, _ptr, u64p
    mono, lag = tables[(64, "honest")]
    for n, code in ((0, ERR_SIZE), (1, ERR_SIZE), (3, ERR_SIZE), (1 << 23, ERR_SIZE)):  # refused before a table is read
        with pytest.raises(BbGpuError, match=code):
            lib.host_srs_lagrange_check(lag, mono, n=n, seed=SEED)
    L = lib.lib
    L.bbgpu_host_srs_lagrange_check.argtypes = [u64p, u64p, C.c_size_t, u64p, C.c_int, C.POINTER(SrsLagrangeCheckReport)]
    rep = SrsLagrangeCheckReport()
    assert L.bbgpu_host_srs_lagrange_check(None, _ptr(mono), 64, _ptr(SEED), 0, C.byref(rep)) == -3
    assert L.bbgpu_host_srs_lagrange_check(_ptr(lag), None, 64, _ptr(SEED), 0, C.byref(rep)) == -3
    assert L.bbgpu_host_srs_lagrange_check(_ptr(lag), _ptr(mono), 64, _ptr(SEED), 0, None) == -3
    assert L.bbgpu_host_srs_lagrange_check(_ptr(lag), _ptr(mono), 64, _ptr(SEED), 2, C.byref(rep)) == -3  # unknown flag bits


def test_device_entry_refuses_its_arguments_before_a_device_is_bound(lib):
    """the GPU entry's verdict on a machine without a GPU: a handle can only exist once a device is bound, so every handle is unknown here"""
    from barretenberg_amd import BbGpuError
    import ctypes as C
    from barretenberg_amd.bbgpu import SrsLagrangeCheckReport, u64p
    for n, code in ((0, ERR_SIZE), (3, ERR_SIZE), (1 << 23, ERR_SIZE), (64, ERR_ARG)):
        with pytest.raises(BbGpuError, match=code):
            lib.srs_lagrange_check(0, 0, n, seed=SEED)
    L = lib.lib
    L.bbgpu_srs_lagrange_check.argtypes = [C.c_int, C.c_int, C.c_size_t, u64p, C.c_int, C.POINTER(SrsLagrangeCheckReport)]
    rep = SrsLagrangeCheckReport()
    assert L.bbgpu_srs_lagrange_check(0, 0, 64, None, 0, None) == -3
    assert L.bbgpu_srs_lagrange_check(0, 0, 64, None, 4, C.byref(rep)) == -3
