"""bbgpu_host_srs_lagrange (csrc/host_srs_lagrange.hpp): the Lagrange-basis conversion of an SRS on the host, for a caller without a GPU -- the definition
the GPU entry's tables and reports are compared with bit for bit (tests/test_gpu_srs_lagrange.py) -- and the butterfly of the GPU kernels run on the CPU.
CPU tests, no GPU.  Expected values are the oracle's (tests/srs_lagrange_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FR, aligned_copy, to_int
from tests.srs_lagrange_cases import (ERR_ARG, ERR_SIZE, NONE, all_g_table, collision_table, generator_times, honest_table, identity_holds, lagrange_at,
                                      omega_table, rows_by_msm, secret_x, tampered, unrelated_points)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def honest(oracle):
    """the honest table of a known x at the largest size: computed once, shared, never written to"""
    x = secret_x(oracle)
    return dict(x=to_int(oracle.from_mont(FR, x)), table=honest_table(oracle, x, 4096))


def clean(rep, n):
    return (rep.n, rep.bad_points, rep.first_bad_point, rep.infinity_rows, rep.first_infinity_row) == (n, 0, NONE, 0, NONE)


@pytest.mark.parametrize("n", [2, 4, 8, 16, 64])
def test_definition(lib, oracle, honest, n):
    """row i of the conversion of the honest table of x is L_i(x) G, odd (endomorphism) entries included"""
    out, rep = lib.host_srs_lagrange(aligned_copy(honest["table"][:2 * n]), n)
    assert np.array_equal(out, generator_times(oracle, lagrange_at(oracle, honest["x"], n)))
    assert clean(rep, n)


@pytest.mark.parametrize("n", [256, 4096])
@pytest.mark.parametrize("kind", ["honest", "unrelated"])
def test_identity(lib, oracle, honest, n, kind):
    """sum_i v_i L_i = sum_j ifft(v)_j P_j"""
    table = aligned_copy(honest["table"][:2 * n]) if kind == "honest" else oracle.point_table(unrelated_points(oracle, n))
    out, rep = lib.host_srs_lagrange(table, n)
    assert clean(rep, n)
    assert identity_holds(oracle, table, out, n, 0x1A6 + n)
    assert np.array_equal(out, oracle.point_table(aligned_copy(out[::2])))  # the odd entries are the endomorphism images of the even ones


def test_in_place(lib, oracle, honest):
    n = 64
    want, _ = lib.host_srs_lagrange(aligned_copy(honest["table"][:2 * n]), n)
    t = aligned_copy(honest["table"][:2 * n])
    out, _ = lib.host_srs_lagrange(t, n, out=t)
    assert out is t and np.array_equal(t, want)


def refused(lib, table, n, match=ERR_ARG):
    """the call is refused and the output untouched; returns the report"""
    from barretenberg_amd import BbGpuError
    sentinel = np.full((2 * n, 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    out = sentinel.copy()
    with pytest.raises(BbGpuError, match=match) as err:
        lib.host_srs_lagrange(table, n, out=out)
    assert np.array_equal(out, sentinel)
    return err.value.report


def test_degenerate_tables(lib, oracle, honest):
    rep = refused(lib, all_g_table(oracle, 8), 8, ERR_ARG + ".*row 1 ")  # x = 1: L_i = delta_i0 G
    assert (rep.n, rep.bad_points, rep.first_bad_point, rep.infinity_rows, rep.first_infinity_row) == (8, 0, NONE, 7, 1)
    rep = refused(lib, omega_table(oracle, 16, 3), 16, ERR_ARG + ".*row 0 ")  # x = omega^3: only row 3 is finite
    assert (rep.infinity_rows, rep.first_infinity_row, rep.bad_points) == (15, 0, 0)
    n = 64
    rep = refused(lib, tampered(honest["table"][:2 * n], 37), n, ERR_ARG + ".*row 37 ")
    assert (rep.n, rep.bad_points, rep.first_bad_point, rep.infinity_rows, rep.first_infinity_row) == (n, 1, 37, 0, NONE)
    rep = refused(lib, tampered(tampered(honest["table"][:2 * n], 5), 60), n)
    assert (rep.bad_points, rep.first_bad_point) == (2, 5)


def test_arguments(lib, oracle, honest):
    from barretenberg_amd import BbGpuError
    table = aligned_copy(honest["table"][:16])
    out = np.zeros((16, 8), dtype=np.uint64)
    for n, code in ((0, ERR_ARG), (1, ERR_SIZE), (3, ERR_SIZE), (1 << 23, ERR_SIZE)):  # refused before the table is read
        with pytest.raises(BbGpuError, match=code):
            lib.host_srs_lagrange(table, n, out=out)
    assert not out.any()


@pytest.mark.parametrize("n,j,j2", [(8, 1, 2), (64, 3, 17)])
def test_collision_tables(lib, oracle, n, j, j2):
    """a doubling and an intermediate infinity in the first stage, every output finite"""
    table = collision_table(oracle, n, j, j2)
    out, rep = lib.host_srs_lagrange(table, n)
    assert clean(rep, n)
    assert identity_holds(oracle, table, out, n, 0xC011 + n)
    if n == 8:
        assert np.array_equal(out[::2], rows_by_msm(oracle, table, n))


def test_device_butterfly_on_the_cpu_under_sanitizers(tmp_path):
    """tests/cpp/test_srs_lagrange_butterfly.hip: the stage kernel's butterfly (the ladder over a projective base, complete additions) as a stand-alone
    host program (own main), the host half built with -fsanitize=address,undefined, against a plain double-and-add and the host group law"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_srs_lagrange_butterfly")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wno-unused-function", "-Wno-pass-failed", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(root, "tests", "cpp", "test_srs_lagrange_butterfly.hip"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
