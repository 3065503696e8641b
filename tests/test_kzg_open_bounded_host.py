"""bbgpu_host_kzg_open_cosets_bounded (csrc/host_kzg_open_cosets.hpp): the m = n / l KZG cell proofs of a polynomial of degree < d by Toeplitz products of
size mu = d / l and one zero-padded forward transform of size m, held to the quotient definition coset by coset (tests/kzg_open_bounded_cases.py) and to
bbgpu_host_kzg_open_cosets over the zero-extended coefficients bit for bit -- the twin the GPU entry is compared with (tests/test_gpu_kzg_open_bounded.py)
-- and the argument verdicts of the twin and of bbgpu_kzg_open_cosets_setup_bounded on a machine without a GPU.  CPU tests."""
import ctypes as C

import numpy as np
import pytest

from tests.kzg_open_bounded_cases import (ERR_ARG, ERR_SIZE, IDENTITY_SHAPES, INF, PAD, bounded_identity_holds, bounded_reference, buffer_of, coset_polynomials,
                                          extended, honest_table, secret_x)

SHAPES = [(8, 2, 4), (16, 1, 4), (32, 4, 8), (64, 4, 32)]  # (n, l, d)
ROWS = 256


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def table(oracle):
    """the honest table of a known x: made once, never written to"""
    return honest_table(oracle, secret_x(oracle), ROWS)


@pytest.mark.parametrize("n,l,d", IDENTITY_SHAPES)
def test_the_bounded_construction_over_plain_integers(oracle, n, l, d):
    """the summed size-2 mu convolution is h, and the size-m transform of the zero-padded h is the quotient commitment on every coset"""
    assert bounded_identity_holds(oracle, n, l, d, 0xB0D + 4096 * n + 64 * l + d)


@pytest.mark.parametrize("n,l,d", SHAPES)
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, PAD)])
def test_twin_against_the_definition_and_the_unbounded_twin(lib, oracle, table, n, l, d, batch, pad):
    """every case polynomial of length d, `batch` of them per call (the list wraps), stride d + pad: all m cosets against synthetic division and
    bbgpu_host_msm_g1 over the zero-extended coefficients, and against bbgpu_host_kzg_open_cosets over them; coefficients and table are read only"""
    cases = coset_polynomials(oracle, d, l)
    rows = table[:2 * n].copy()
    stride = d + pad
    for k in range(0, len(cases), batch):
        group = [cases[(k + b) % len(cases)] for b in range(batch)]
        buf = buffer_of(oracle, [c for _, c in group], stride)
        kept = buf.copy()
        got = lib.host_kzg_open_cosets(rows, n, l, buf, batch=batch, stride=stride, degree_bound=d)
        assert got.shape == (batch, n // l, 8) and np.array_equal(buf, kept)
        old = lib.host_kzg_open_cosets(rows, n, l, np.concatenate([extended(c, n) for _, c in group]), batch=batch)
        assert np.array_equal(got, old)
        if batch == 1:
            assert np.array_equal(got[0], bounded_reference(lib, oracle, table, group[0][1], n, l)), group[0][0]
    assert np.array_equal(rows, table[:2 * n])
    if l > 1:
        for name in ("degree < l", "last level cancels"):
            assert np.array_equal(lib.host_kzg_open_cosets(rows, n, l, dict(cases)[name], degree_bound=d)[0], np.tile(INF, (n // l, 1))), name


def test_a_full_wave_of_residues_over_the_shortest_product(lib, oracle, table):
    """(256, 64, 128): mu = 2, M = 4, l = 64 -- every case against the unbounded twin, a handful of cosets of two of them against the definition"""
    n, l, d = 256, 64, 128
    cases = coset_polynomials(oracle, d, l)
    rows = table[:2 * n].copy()
    got = lib.host_kzg_open_cosets(rows, n, l, buffer_of(oracle, [c for _, c in cases], d + PAD), batch=len(cases), stride=d + PAD, degree_bound=d)
    assert np.array_equal(got, lib.host_kzg_open_cosets(rows, n, l, np.concatenate([extended(c, n) for _, c in cases]), batch=len(cases)))
    picks = [0, 1, 2, 3]  # m = 4: all of them
    for b in (0, len(cases) - 2):  # random; last level doubles
        assert np.array_equal(got[b][picks], bounded_reference(lib, oracle, table, cases[b][1], n, l, cosets=picks)), cases[b][0]


@pytest.mark.parametrize("n,l", [(8, 4), (64, 1)])
def test_a_bound_of_n_is_the_twin_without_one(lib, oracle, table, n, l):
    rows = table[:2 * n].copy()
    cases = coset_polynomials(oracle, n, l)
    buf = buffer_of(oracle, [c for _, c in cases], n + PAD)
    assert np.array_equal(lib.host_kzg_open_cosets(rows, n, l, buf, batch=len(cases), stride=n + PAD, degree_bound=n),
                          lib.host_kzg_open_cosets(rows, n, l, buf, batch=len(cases), stride=n + PAD))


def test_coefficients_from_d_on_are_not_read(lib, oracle, table):
    """(32, 4, 8): what lies at [d, stride) changes nothing, whether the stride is n, more, or exactly d with the polynomials back to back"""
    n, l, d = 32, 4, 8
    rows = table[:2 * n].copy()
    polys = [c for _, c in coset_polynomials(oracle, d, l)[:3]]
    want = lib.host_kzg_open_cosets(rows, n, l, np.concatenate([extended(c, n) for c in polys]), batch=3, degree_bound=d)  # zeros from d on
    for stride in (n, n + PAD):
        buf = buffer_of(oracle, polys, stride)  # other values from d on
        assert np.any(buf[d:stride]) and np.array_equal(lib.host_kzg_open_cosets(rows, n, l, buf, batch=3, stride=stride, degree_bound=d), want), stride
    back_to_back = np.concatenate(polys)
    assert back_to_back.shape == (3 * d, 4)
    assert np.array_equal(lib.host_kzg_open_cosets(rows, n, l, back_to_back, batch=3, stride=d, degree_bound=d), want)


def test_a_table_of_exactly_d_rows_is_accepted(lib, oracle, table):
    """(16, 2, 8) over the first 8 rows alone; a row off the curve below d - l is named, a row from d - l on is not read"""
    n, l, d = 16, 2, 8
    c = buffer_of(oracle, [p for _, p in coset_polynomials(oracle, d, l)[:2]], d)
    short = table[:2 * d].copy()
    assert short.shape == (2 * d, 8)
    want = lib.host_kzg_open_cosets(table[:2 * n].copy(), n, l, c, batch=2, stride=d, degree_bound=d)
    assert np.array_equal(lib.host_kzg_open_cosets(short, n, l, c, batch=2, stride=d, degree_bound=d), want)
    assert np.array_equal(want[0], bounded_reference(lib, oracle, table, c[:d], n, l))
    from barretenberg_amd import BbGpuError
    bad = short.copy()
    bad[2 * 3, 4] ^= 1  # row 3 leaves the curve
    bad[2 * 5, 4] ^= 1  # and row 5: the first one is named
    with pytest.raises(BbGpuError, match=ERR_ARG + ".*row 3 "):
        lib.host_kzg_open_cosets(bad, n, l, c, batch=2, stride=d, degree_bound=d)
    last_read = short.copy()
    last_read[2 * (d - l - 1), 4] ^= 1
    with pytest.raises(BbGpuError, match=ERR_ARG + ".*row %d " % (d - l - 1)):
        lib.host_kzg_open_cosets(last_read, n, l, c, batch=2, stride=d, degree_bound=d)
    for row in range(d - l, d):
        unread = short.copy()
        unread[2 * row] = 0
        assert np.array_equal(lib.host_kzg_open_cosets(unread, n, l, c, batch=2, stride=d, degree_bound=d), want), row


def test_twin_refusals(lib, oracle, table):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import _ptr, u64p
    n, l, d = 32, 4, 8
    rows, c = table[:2 * n].copy(), buffer_of(oracle, [p for _, p in coset_polynomials(oracle, d, l)[:2]], n)
    for kw in (dict(d=0), dict(d=12), dict(d=24), dict(d=l), dict(d=l // 2), dict(d=1), dict(d=2 * n), dict(d=1 << 22),  # not a power of two, < 2 l, > n
               dict(d=d, stride=d - 1), dict(d=n, stride=n - 1), dict(d=d, batch=0), dict(d=d, batch=65), dict(n=12, d=8), dict(n=n, l=3, d=8)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.host_kzg_open_cosets(rows, kw.get("n", n), kw.get("l", l), c, batch=kw.get("batch", 2), stride=kw.get("stride", n), degree_bound=kw["d"])
    big = np.zeros((4, 4), dtype=np.uint64)  # batch x 2 n above 2^22 whatever d is: judged before anything is read
    with pytest.raises(BbGpuError, match=ERR_SIZE):
        lib.host_kzg_open_cosets(rows, 1 << 21, 64, big, batch=2, stride=128, degree_bound=128)
    L = lib.lib
    L.bbgpu_host_kzg_open_cosets_bounded.argtypes = [u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p]
    out = np.zeros((2, n // l, 8), dtype=np.uint64)
    for args in ((None, n, l, d, _ptr(c), n, 2, _ptr(out)), (_ptr(rows), n, l, d, None, n, 2, _ptr(out)), (_ptr(rows), n, l, d, _ptr(c), n, 2, None)):
        assert L.bbgpu_host_kzg_open_cosets_bounded(*args) == -3
    assert L.bbgpu_host_kzg_open_cosets_bounded(_ptr(rows), n, l, d, _ptr(c), n, 2, _ptr(out)) == 0


def test_the_bounded_setup_refuses_its_arguments_before_a_device_is_bound(lib):
    """every argument error of bbgpu_kzg_open_cosets_setup_bounded that needs no live handle, on a machine without a GPU.  (Those that need a table or a
    setup -- d above the table, the stride below d, the pool -- are in tests/test_gpu_kzg_open_bounded.py.)"""
    from barretenberg_amd import BbGpuError
    for n, l, d in ((32, 4, 0), (32, 4, 12), (32, 4, 4), (32, 4, 2), (32, 4, 64), (32, 1, 1), (32, 1, 3), (1 << 21, 64, 64), (1 << 21, 64, 1 << 22),
                    (12, 4, 8), (32, 3, 8), (1 << 22, 64, 128), (256, 128, 256)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_setup(0, n, l, degree_bound=d)
    for handle in (-1, 0, 1 << 20):  # no table is registered
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_cosets_setup(handle, 32, 4, degree_bound=8)
