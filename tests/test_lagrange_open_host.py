"""bbgpu_host_fr_evaluate_lagrange / bbgpu_host_kate_opening_lagrange (csrc/host_lagrange_open.hpp): evaluation and opening of polynomials given by their
values on the domain, on the host -- the definition the GPU entries are compared with bit for bit (tests/test_gpu_lagrange_open.py).  CPU tests, no GPU.
Expected values are the oracle's, through the coefficient form (tests/lagrange_open_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests.lagrange_open_cases import ERR_ARG, ERR_SIZE, PAD, expected_batch, values, z_cases

SIZES = [2, 4, 8, 64, 256]


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, 0), (3, 5)])
def test_definition(lib, oracle, n, batch, pad):
    """f(z) and the quotient against the coefficient form, at every kind of z; the elements between the polynomials stay as they were; in place"""
    stride = n + pad
    v = values(oracle, 0xE7A1 + n + batch, n, batch, stride)
    kept = v.copy()
    for name, z, _ in z_cases(oracle, n):
        f_want, q_want = expected_batch(oracle, v, n, batch, stride, z)
        assert np.array_equal(lib.host_evaluate_lagrange(v, z, n=n, batch=batch, stride=stride), f_want), name
        q, f = lib.host_kate_opening_lagrange(v, z, n=n, batch=batch, stride=stride)
        assert np.array_equal(f, f_want) and np.array_equal(q, q_want), name
        assert np.array_equal(v, kept), name
        w = v.copy()
        q2, f2 = lib.host_kate_opening_lagrange(w, z, n=n, batch=batch, stride=stride, out=w)  # in place
        assert q2 is w and np.array_equal(w, q_want) and np.array_equal(f2, f_want), name
    if pad:
        assert (q_want.reshape(batch, stride, 4)[:, n:] == PAD).all()


def test_the_cases_reach_both_paths(oracle):
    for n in SIZES:
        ms = [m for _, _, m in z_cases(oracle, n)]
        assert None in ms and 0 in ms and n - 1 in ms and n // 2 in ms


def test_arguments(lib, oracle):
    from barretenberg_amd import BbGpuError
    import ctypes as C
    n = 8
    v = values(oracle, 1, n, 2, n)
    z = oracle.random_scalars(2, 1)[0]
    for kw, code in ((dict(n=0), ERR_SIZE), (dict(n=1), ERR_SIZE), (dict(n=3), ERR_SIZE), (dict(n=1 << 25), ERR_SIZE), (dict(n=n, batch=0), ERR_SIZE),
                     (dict(n=n, batch=65), ERR_SIZE), (dict(n=n, batch=2, stride=n - 1), ERR_SIZE)):
        kw = dict(dict(batch=1, stride=max(kw.get("n", n), 1)), **kw)
        with pytest.raises(BbGpuError, match=code):
            lib.host_evaluate_lagrange(v, z, **kw)
        out = v.copy()
        with pytest.raises(BbGpuError, match=code):
            lib.host_kate_opening_lagrange(v, z, out=out, **kw)
        assert np.array_equal(out, v)
    # null pointers, straight through the C ABI
    L = lib.lib
    from barretenberg_amd.bbgpu import _ptr, u64p
    L.bbgpu_host_fr_evaluate_lagrange.argtypes = [u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p]
    L.bbgpu_host_kate_opening_lagrange.argtypes = [u64p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p]
    out = np.zeros((2, 4), dtype=np.uint64)
    q = v.copy()
    for args in ((None, n, n, 2, _ptr(z), _ptr(out)), (_ptr(v), n, n, 2, None, _ptr(out)), (_ptr(v), n, n, 2, _ptr(z), None)):
        assert L.bbgpu_host_fr_evaluate_lagrange(*args) == -3
    for args in ((None, _ptr(q), n, n, 2, _ptr(z), _ptr(out)), (_ptr(v), None, n, n, 2, _ptr(z), _ptr(out)), (_ptr(v), _ptr(q), n, n, 2, None, _ptr(out))):
        assert L.bbgpu_host_kate_opening_lagrange(*args) == -3
    assert L.bbgpu_host_kate_opening_lagrange(_ptr(v), _ptr(q), n, n, 2, _ptr(z), None) == 0  # f_of_z may be NULL
    assert np.array_equal(q, lib.host_kate_opening_lagrange(v, z, n=n, batch=2, stride=n)[0])


def test_device_entries_refuse_their_arguments_before_a_device_is_bound(lib, oracle):
    """the same verdict from the two GPU entries, on a machine without a GPU: nothing is initialised for a call that is refused"""
    from barretenberg_amd import BbGpuError
    z = oracle.random_scalars(2, 1)[0]
    fake = 0x1000  # never dereferenced
    for kw, code in ((dict(n=0), ERR_SIZE), (dict(n=3), ERR_SIZE), (dict(n=1 << 25), ERR_SIZE), (dict(n=8, batch=0), ERR_SIZE), (dict(n=8, batch=65), ERR_SIZE),
                     (dict(n=8, stride=7), ERR_SIZE)):
        with pytest.raises(BbGpuError, match=code):
            lib.evaluate_lagrange_device(fake, z=z, **kw)
        with pytest.raises(BbGpuError, match=code):
            lib.kate_opening_lagrange_device(fake, fake, z=z, **kw)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.evaluate_lagrange_device(None, 8, z)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kate_opening_lagrange_device(None, fake, 8, z)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kate_opening_lagrange_device(fake, None, 8, z)


def test_host_twins_under_sanitizers(tmp_path):
    """tests/cpp/test_lagrange_open_host.cpp: both host twins as a stand-alone program (own main) built with -fsanitize=address,undefined: n = 2 and 64,
    on and off the domain, in place and with padding, against Horner evaluation and synthetic division of the interpolated coefficients"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_lagrange_open_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_lagrange_open_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
