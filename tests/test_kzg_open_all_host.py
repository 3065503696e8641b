"""bbgpu_host_kzg_open_all (csrc/host_kzg_open_all.hpp; the twin of csrc/host_kzg_open_cosets.hpp at coset size 1): the n KZG proofs of a polynomial at every point of its domain by one Toeplitz product and one group
transform, held to the quotient definition point by point (tests/kzg_open_all_cases.py: bbgpu_host_kate_opening, then bbgpu_host_msm_g1) -- the twin the GPU
entry is compared with bit for bit (tests/test_gpu_kzg_open_all.py) -- and the argument verdicts of the twin and of the device entries on a machine
without a GPU.  CPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.kzg_open_all_cases import (ERR_ARG, ERR_SIZE, INF, PAD, buffer_of, honest_table, infinite_row_table, polynomials, reference, secret_x,
                                      toeplitz_identity_holds)

SIZES = [2, 4, 8, 64]


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def world(lib, oracle):
    """the honest table of a known x and, per (n, polynomial), the proofs by the quotient definition: made once, never written to"""
    table = honest_table(oracle, secret_x(oracle), max(SIZES))
    made = {}

    def want(n, name, coeffs):
        if (n, name) not in made:
            made[(n, name)] = reference(lib, oracle, table, coeffs)
        return made[(n, name)]
    return dict(table=table, want=want)


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_the_construction_over_plain_integers(oracle, n):
    """the forward transform of h is the quotient commitment at every point, and the cyclic convolution of s and t is h"""
    assert toeplitz_identity_holds(oracle, n, 0x70E9 + n)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, 0), (3, PAD)])
def test_twin_against_the_definition(lib, oracle, world, n, batch, pad):
    """every polynomial of the cases module, `batch` of them per call; the coefficients and the table are read only"""
    cases = polynomials(oracle, n)
    table = world["table"][:2 * n].copy()
    stride = n + pad
    for k in range(0, len(cases), batch):
        group = [cases[(k + b) % len(cases)] for b in range(batch)]
        buf = buffer_of(oracle, [c for _, c in group], stride)
        kept = buf.copy()
        got = lib.host_kzg_open_all(table, n, buf, batch=batch, stride=stride)
        assert got.shape == (batch, n, 8)
        for b, (name, c) in enumerate(group):
            assert np.array_equal(got[b], world["want"](n, name, c)), (name, b)
        assert np.array_equal(buf, kept)
    assert np.array_equal(table, world["table"][:2 * n])


@pytest.mark.parametrize("n", SIZES)
def test_the_proofs_that_are_known_without_a_reference(lib, oracle, world, n):
    cases = dict(polynomials(oracle, n))
    table = world["table"][:2 * n].copy()
    for name in ("zero", "constant"):
        assert np.array_equal(lib.host_kzg_open_all(table, n, cases[name])[0], np.tile(INF, (n, 1))), name
    assert np.array_equal(lib.host_kzg_open_all(table, n, cases["X"])[0], np.tile(table[0], (n, 1)))


def test_a_string_whose_transform_has_a_row_at_infinity(lib, oracle):
    """x = W zeta at n = 4: row 1 of S^ is the point at infinity, an intermediate the twin keeps; the proofs are those of the definition"""
    table = infinite_row_table(oracle)
    for name, c in polynomials(oracle, 4):
        assert np.array_equal(lib.host_kzg_open_all(table, 4, c)[0], reference(lib, oracle, table, c)), name


def test_twin_arguments(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import _ptr, u64p
    n = 8
    table, c = world["table"][:2 * n].copy(), buffer_of(oracle, [p for _, p in polynomials(oracle, n)[:2]], n)
    big = np.zeros((4, 4), dtype=np.uint64)  # sizes are judged before anything is read
    for kw in (dict(n=0), dict(n=1), dict(n=3), dict(n=12), dict(n=1 << 22), dict(n=n, batch=0), dict(n=n, batch=65), dict(n=n, batch=2, stride=n - 1),
               dict(n=1 << 21, batch=2, stride=1 << 21), dict(n=1 << 16, batch=64, stride=1 << 16)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.host_kzg_open_all(table, kw["n"], big if kw["n"] != n else c, batch=kw.get("batch", 1), stride=kw.get("stride", kw["n"]))
    L = lib.lib
    L.bbgpu_host_kzg_open_all.argtypes = [u64p, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p]
    out = np.zeros((2, n, 8), dtype=np.uint64)
    for args in ((None, n, _ptr(c), n, 2, _ptr(out)), (_ptr(table), n, None, n, 2, _ptr(out)), (_ptr(table), n, _ptr(c), n, 2, None)):
        assert L.bbgpu_host_kzg_open_all(*args) == -3
    bad = table.copy()
    bad[2 * 5, 4] ^= 1  # row 5 leaves the curve; row n - 1 = 7 is not read
    with pytest.raises(BbGpuError, match=ERR_ARG + ".*row 5 "):
        lib.host_kzg_open_all(bad, n, c, batch=2)
    unread = table.copy()
    unread[2 * 7] = 0
    assert np.array_equal(lib.host_kzg_open_all(unread, n, c, batch=2), lib.host_kzg_open_all(table, n, c, batch=2))


def test_device_entries_refuse_their_arguments_before_a_device_is_bound(lib):
    """every argument error of the device entries that needs no live handle, on a machine without a GPU: nothing is initialised for a call that is
    refused.  (The verdicts that need a table or a setup -- n above the table, the stride, batch x 2 n -- are in tests/test_gpu_kzg_open_all.py.)"""
    from barretenberg_amd import BbGpuError
    fake = 0x1000  # never dereferenced
    for n in (0, 1, 3, 12, 1 << 22, 1 << 23):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_all_setup(0, n)
    for handle in (-1, 0, 1 << 20):  # no table is registered
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_all_setup(handle, 8)
    for setup in (-1, 0, 15, 16):  # no setup exists
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_all_release(setup)
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_all_device(setup, fake, 8)
    for batch in (0, -1, 65):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_all_device(0, fake, 8, batch=batch)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kzg_open_all_device(0, None, 8)
    L = lib.lib
    L.bbgpu_kzg_open_all_device.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    assert L.bbgpu_kzg_open_all_device(0, fake, 8, 1, None, None) == -3


def test_host_twin_under_sanitizers(tmp_path):
    """tests/cpp/test_kzg_open_all_host.cpp: the twin as a stand-alone program (own main) built with -fsanitize=address,undefined: n = 8 and 64, batch 1
    and 3 with padding, against the quotient definition"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kzg_open_all_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_kzg_open_all_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
