"""bbgpu_host_kzg_open_cosets (csrc/host_kzg_open_cosets.hpp): the m = n / l KZG cell proofs of a polynomial, one per coset of its domain, by l Toeplitz
products summed in the Fourier domain and one group transform, held to the quotient definition coset by coset (tests/kzg_open_cosets_cases.py: synthetic
division over Python integers, then bbgpu_host_msm_g1) -- the twin the GPU entry is compared with bit for bit (tests/test_gpu_kzg_open_cosets.py) -- and the
argument verdicts of the twin and of the device entries on a machine without a GPU.  CPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.kzg_open_cosets_cases import (ERR_ARG, ERR_SIZE, INF, PAD, buffer_of, coset_polynomials, cosets_identity_holds, fold_single_proofs, honest_table,
                                         reference, secret_x)

SIZES = [(4, 2), (8, 2), (8, 4), (16, 4), (64, 16), (128, 64)]


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def world(lib, oracle):
    """the honest table of a known x and, per (n, l, polynomial), the proofs by the quotient definition: made once, never written to"""
    table = honest_table(oracle, secret_x(oracle), max(n for n, _ in SIZES))
    made = {}

    def want(n, l, name, coeffs):
        if (n, l, name) not in made:
            made[(n, l, name)] = reference(lib, oracle, table, coeffs, l)
        return made[(n, l, name)]
    return dict(table=table, want=want)


@pytest.mark.parametrize("n,l", [(4, 2), (8, 4), (16, 1), (32, 8)])
def test_the_construction_over_plain_integers(oracle, n, l):
    """the transform of h is the quotient commitment on every coset, the summed convolution is h, and the proofs are the partial-fraction folds"""
    assert cosets_identity_holds(oracle, n, l, 0xC05E7 + 64 * n + l)


@pytest.mark.parametrize("n,l", SIZES)
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, PAD)])
def test_twin_against_the_definition(lib, oracle, world, n, l, batch, pad):
    """every case polynomial, `batch` of them per call (the list wraps); the coefficients and the table are read only"""
    cases = coset_polynomials(oracle, n, l)
    table = world["table"][:2 * n].copy()
    stride = n + pad
    for k in range(0, len(cases), batch):
        group = [cases[(k + b) % len(cases)] for b in range(batch)]
        buf = buffer_of(oracle, [c for _, c in group], stride)
        kept = buf.copy()
        got = lib.host_kzg_open_cosets(table, n, l, buf, batch=batch, stride=stride)
        assert got.shape == (batch, n // l, 8)
        for b, (name, c) in enumerate(group):
            assert np.array_equal(got[b], world["want"](n, l, name, c)), (name, b)
        assert np.array_equal(buf, kept)
    assert np.array_equal(table, world["table"][:2 * n])
    for name in ("degree < l", "last level cancels"):
        assert np.array_equal(world["want"](n, l, name, dict(cases)[name]), np.tile(INF, (n // l, 1))), name


@pytest.mark.parametrize("n", [2, 4, 16])
def test_cosets_of_one_point_are_the_single_proofs(lib, oracle, world, n):
    table = world["table"][:2 * n].copy()
    buf = buffer_of(oracle, [c for _, c in coset_polynomials(oracle, n, 1)], n + PAD)
    batch = buf.shape[0] // (n + PAD)
    assert np.array_equal(lib.host_kzg_open_cosets(table, n, 1, buf, batch=batch, stride=n + PAD), lib.host_kzg_open_all(table, n, buf, batch=batch, stride=n + PAD))


def test_twin_against_the_fold_of_the_single_proofs(lib, oracle, world):
    """(16, 4): pi_k = sum_j [omega^(k + m j) / (l psi^k)] pi(omega^(k + m j)) over bbgpu_host_kzg_open_all's proofs"""
    n, l = 16, 4
    table, c = world["table"][:2 * n].copy(), coset_polynomials(oracle, n, l)[0][1]
    singles = lib.host_kzg_open_all(table, n, c)[0]
    assert np.array_equal(lib.host_kzg_open_cosets(table, n, l, c)[0], fold_single_proofs(lib, oracle, singles, n, l))


def test_twin_arguments(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import _ptr, u64p
    n, l = 16, 4
    table, c = world["table"][:2 * n].copy(), buffer_of(oracle, [p for _, p in coset_polynomials(oracle, n, l)[:2]], n)
    big = np.zeros((4, 4), dtype=np.uint64)  # sizes are judged before anything is read
    for kw in (dict(n=0), dict(n=1), dict(n=3), dict(n=12), dict(n=1 << 22), dict(n=n, l=0), dict(n=n, l=3), dict(n=n, l=n), dict(n=n, l=2 * n), dict(n=256, l=128),
               dict(n=n, batch=0), dict(n=n, batch=65), dict(n=n, batch=2, stride=n - 1), dict(n=1 << 21, l=64, batch=2, stride=1 << 21),
               dict(n=1 << 16, l=64, batch=64, stride=1 << 16)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.host_kzg_open_cosets(table, kw["n"], kw.get("l", l), big if kw["n"] != n else c, batch=kw.get("batch", 1), stride=kw.get("stride", kw["n"]))
    L = lib.lib
    L.bbgpu_host_kzg_open_cosets.argtypes = [u64p, C.c_size_t, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p]
    out = np.zeros((2, n // l, 8), dtype=np.uint64)
    for args in ((None, n, l, _ptr(c), n, 2, _ptr(out)), (_ptr(table), n, l, None, n, 2, _ptr(out)), (_ptr(table), n, l, _ptr(c), n, 2, None)):
        assert L.bbgpu_host_kzg_open_cosets(*args) == -3
    bad = table.copy()
    bad[2 * 5, 4] ^= 1  # row 5 leaves the curve
    bad[2 * 9, 4] ^= 1  # and row 9: the first one is named
    with pytest.raises(BbGpuError, match=ERR_ARG + ".*row 5 "):
        lib.host_kzg_open_cosets(bad, n, l, c, batch=2)
    want = lib.host_kzg_open_cosets(table, n, l, c, batch=2)
    for row in range(n - l, n):  # rows from n - l on are not read
        unread = table.copy()
        unread[2 * row] = 0
        assert np.array_equal(lib.host_kzg_open_cosets(unread, n, l, c, batch=2), want), row
    last_read = table.copy()
    last_read[2 * (n - l - 1), 4] ^= 1
    with pytest.raises(BbGpuError, match=ERR_ARG + ".*row %d " % (n - l - 1)):
        lib.host_kzg_open_cosets(last_read, n, l, c, batch=2)


def test_device_entries_refuse_their_arguments_before_a_device_is_bound(lib):
    """every argument error of the device entries that needs no live handle, on a machine without a GPU: nothing is initialised for a call that is
    refused.  (The verdicts that need a table or a setup -- n above the table, the stride, batch x 2 n, the pool -- are in
    tests/test_gpu_kzg_open_cosets.py.)"""
    from barretenberg_amd import BbGpuError
    fake = 0x1000  # never dereferenced
    for n, l in ((0, 1), (1, 1), (3, 1), (12, 4), (1 << 22, 64), (16, 0), (16, 3), (16, 16), (16, 32), (256, 128), (2, 2)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_setup(0, n, l)
    for handle in (-1, 0, 1 << 20):  # no table is registered
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_cosets_setup(handle, 8, 2)
    for setup in (-1, 0, 15, 16):  # no setup exists
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_cosets_release(setup)
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_cosets_device(setup, fake, 8, 2)
    for batch in (0, -1, 65):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_device(0, fake, 8, 2, batch=batch)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kzg_open_cosets_device(0, None, 8, 2)
    L = lib.lib
    L.bbgpu_kzg_open_cosets_device.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    assert L.bbgpu_kzg_open_cosets_device(0, fake, 8, 1, None, None) == -3


def test_host_twin_under_sanitizers(tmp_path):
    """tests/cpp/test_kzg_open_cosets_host.cpp: the twin as a stand-alone program (own main) built with -fsanitize=address,undefined: (8, 2), (16, 4) and
    (128, 64), batch 1 and 3 with padding, against the quotient definition"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kzg_open_cosets_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_kzg_open_cosets_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
