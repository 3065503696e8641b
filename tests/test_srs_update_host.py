"""bbgpu_host_srs_update, bbgpu_host_srs_update_check and bbgpu_transcript_write_g2 (csrc/host_srs_update.hpp): the SRS update on the host, for a caller
without a GPU -- the definition the GPU entry's tables and reports are compared with bit for bit (tests/test_gpu_srs_update.py).  CPU tests, no GPU.
Expected values are the oracle's (tests/srs_update_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FQ, FR, FR_MODULUS as R, aligned_copy, from_int, to_int
from tests.srs_check_cases import SEED, g2_of
from tests.srs_update_cases import (NONE, all_g_table, check_split, honest_table, lam, mont, row_times, row_times_plain, rows_times_powers, secret_x, secret_y, special_ys,
                                    split_cases, tampered, unrelated_points, updated_table)

SIZES = [1, 2, 300, 1000]


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def world(lib, oracle, tmp_path_factory):
    """the secrets, the honest table of x and its update by y at the largest size, x G2 and (x y) G2: computed once, shared, never written to"""
    tmp = tmp_path_factory.mktemp("srs_update")
    x, y = secret_x(oracle), secret_y(oracle)
    xy = oracle.mul(FR, x, y)
    return dict(x=x, y=y, xy=xy, table=honest_table(oracle, x, 1000), want=updated_table(oracle, x, y, 1000), g2_x=g2_of(lib, oracle, tmp, x, "x.dat"),
                g2_xy=g2_of(lib, oracle, tmp, xy, "xy.dat"), tmp=tmp)


def test_endomorphism_image_is_minus_lambda_p(oracle, world):
    """what the device ladder builds on: the odd table entry (beta x, -y) is -lambda P under the repository's beta and the lambda of the split"""
    L = lam(oracle)
    assert pow(L, 3, R) == 1 and L != 1
    for i in (1, 2, 999):
        minus_lambda_p = row_times(oracle, world["table"][2 * i], mont(oracle, R - L))
        assert np.array_equal(minus_lambda_p, world["table"][2 * i + 1])


def test_split_on_the_host(lib, oracle, golden):
    """the 64-bit integer split of csrc/srs_update.hip, run on the host: the golden values of tests/golden/endo_wnaf.json, and a split of every other scalar"""
    pinned, free = split_cases(oracle, golden)
    ks = np.array([from_int(k) for k, _, _ in pinned] + [from_int(k) for k in free], dtype=np.uint64)
    check_split(oracle, pinned, free, lib.selftest_endo_split(ks, on_device=False))


@pytest.mark.parametrize("n", SIZES)
def test_powers_table(lib, oracle, world, n):
    out, rep = lib.host_srs_update(aligned_copy(world["table"][:2 * n]), n, world["y"])
    assert np.array_equal(out, world["want"][:2 * n])  # odd (endomorphism) entries included
    assert (rep.n, rep.first_power, rep.bad_points, rep.first_bad_point, rep.g2_ok) == (n, 0, 0, NONE, 0)
    assert not any(rep.g2_x_out)


def test_bit_walk(lib, oracle, world):
    """y = 2 over 300 rows: the set bit of the scalar walks through every window boundary, and from row 254 on the power wraps modulo r"""
    two = mont(oracle, 2)
    out, _ = lib.host_srs_update(aligned_copy(world["table"][:600]), 300, two)
    assert np.array_equal(out, updated_table(oracle, world["x"], two, 300))


def test_all_g_table(lib, oracle, world):
    out, _ = lib.host_srs_update(all_g_table(oracle, 300), 300, world["y"])
    assert np.array_equal(out, honest_table(oracle, world["y"], 300))


def test_unrelated_rows(lib, oracle, world):
    pts = unrelated_points(oracle, 24)
    out, _ = lib.host_srs_update(oracle.point_table(pts), 24, world["y"], first=3)
    assert np.array_equal(out, rows_times_powers(oracle, pts, world["y"], first=3))


def test_single_rows_special_scalars(lib, oracle):
    p = unrelated_points(oracle, 3)[1:2]
    table = oracle.point_table(aligned_copy(p))
    for name, y in special_ys(oracle):
        out, rep = lib.host_srs_update(table, 1, y, first=1)
        assert np.array_equal(out[0], row_times_plain(oracle, p[0], y)), name
        assert name == "negative-t" or np.array_equal(out[0], row_times(oracle, p[0], y)), name
        assert rep.first_power == 1
    same, _ = lib.host_srs_update(table, 1, mont(oracle, 1), first=1)
    assert np.array_equal(same, table)  # y = 1 copies


def test_offsets(lib, oracle, world):
    n = 300
    tail, rep = lib.host_srs_update(aligned_copy(world["table"][10:2 * n]), n - 5, world["y"], first=5)
    assert np.array_equal(tail, world["want"][10:2 * n]) and rep.first_power == 5 and rep.n == n - 5


def test_composition(lib, oracle, world):
    n = 64
    y2 = oracle.random_scalars(0x2222, 1)[0]
    once, _ = lib.host_srs_update(aligned_copy(world["table"][:2 * n]), n, world["y"])
    twice, _ = lib.host_srs_update(once, n, y2)
    both, _ = lib.host_srs_update(aligned_copy(world["table"][:2 * n]), n, oracle.mul(FR, world["y"], y2))
    assert np.array_equal(twice, both)
    assert np.array_equal(twice, updated_table(oracle, world["x"], oracle.mul(FR, world["y"], y2), n))


def test_in_place(lib, oracle, world):
    n = 300
    t = aligned_copy(world["table"][:2 * n])
    out, _ = lib.host_srs_update(t, n, world["y"], out=t)
    assert out is t and np.array_equal(t, world["want"][:2 * n])


def test_g2_half(lib, oracle, world):
    n = 64
    table = aligned_copy(world["table"][:2 * n])
    out, rep = lib.host_srs_update(table, n, world["y"], world["g2_x"])
    g2_out, y_g2 = np.array(rep.g2_x_out, dtype=np.uint64), np.array(rep.y_g2, dtype=np.uint64)
    assert rep.g2_ok == 1 and np.array_equal(g2_out, world["g2_xy"])  # the x G2 of x y, from a transcript written with that secret
    assert np.array_equal(y_g2, g2_of(lib, oracle, world["tmp"], world["y"], "y.dat"))
    assert lib.host_srs_check(out, n, g2_out, SEED).ok
    old = lib.host_srs_check(out, n, world["g2_x"], SEED)
    assert old.powers_checked == 1 and old.powers_ok == 0
    one, rep1 = lib.host_srs_update(table, n, mont(oracle, 1), world["g2_x"])
    assert np.array_equal(np.array(rep1.g2_x_out, dtype=np.uint64), world["g2_x"]) and lib.host_srs_check(one, n, world["g2_x"], SEED).ok  # y = 1
    # only the first power enters G2, whatever first_power
    _, rep5 = lib.host_srs_update(aligned_copy(table[10:]), n - 5, world["y"], world["g2_x"], first=5)
    assert np.array_equal(np.array(rep5.g2_x_out, dtype=np.uint64), world["g2_xy"])
    # the proof of the update
    assert lib.host_srs_update_check(table[2], out[2], y_g2)
    other, _ = lib.host_srs_update(table, n, oracle.random_scalars(0x3333, 1)[0])
    assert not lib.host_srs_update_check(table[2], other[2], y_g2)
    off_twist = y_g2.copy()
    off_twist[8:12] = from_int((to_int(off_twist[8:12]) + 1) % (1 << 256))
    assert not lib.host_srs_update_check(table[2], out[2], off_twist)
    # a bad x G2: no G2 half
    _, bad = lib.host_srs_update(table, n, world["y"], off_twist)
    assert bad.g2_ok == 0 and not any(bad.g2_x_out) and np.array_equal(np.array(bad.y_g2, dtype=np.uint64), y_g2)


def test_transcript_round_trip(lib, oracle, world, tmp_path):
    n = 64
    out, rep = lib.host_srs_update(aligned_copy(world["table"][:2 * n]), n, world["y"], world["g2_x"])
    g2_out = np.array(rep.g2_x_out, dtype=np.uint64)
    path = str(tmp_path / "updated.dat")
    lib.write_transcript_g2(path, out, n, g2_out)
    assert np.array_equal(lib.read_transcript(path, n), out)
    assert np.array_equal(lib.transcript_read_g2(path), g2_out)
    with open(path, "rb") as a:  # byte for byte the file the holder of x y would write
        secret_path = str(tmp_path / "secret.dat")
        lib.write_transcript(secret_path, out, n, world["xy"])
        with open(secret_path, "rb") as b:
            assert a.read() == b.read()
    from barretenberg_amd import BbGpuError
    bad = g2_out.copy()
    bad[8:12] = from_int((to_int(bad[8:12]) + 1) % (1 << 256))
    with pytest.raises(BbGpuError, match=" -3:"):
        lib.write_transcript_g2(path, out, n, bad)


def test_refusals(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    n = 300
    table = aligned_copy(world["table"][:2 * n])
    for bad_y in (np.zeros(4, dtype=np.uint64), from_int(R), None):  # y == 0 given as 0 and as r; a null y
        with pytest.raises(BbGpuError, match=" -3:"):
            lib.host_srs_update(table, n, bad_y)
    with pytest.raises(BbGpuError, match=" -3:"):
        lib.host_srs_update(table, 0, world["y"])
    with pytest.raises(BbGpuError, match=" -3:"):
        lib.host_srs_update(table, n, world["y"], first=(1 << 32) - n + 1)
    for k in (0, n // 2, n - 1):
        t = tampered(table, k)
        sentinel = np.full((2 * n, 8), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        out = sentinel.copy()
        with pytest.raises(BbGpuError, match=" -3:.*row %d " % k) as err:
            lib.host_srs_update(t, n, world["y"], out=out)
        rep = err.value.report
        assert (rep.n, rep.bad_points, rep.first_bad_point) == (n, 1, k)
        assert np.array_equal(out, sentinel)  # untouched
    t = tampered(tampered(table, 7), 200)
    with pytest.raises(BbGpuError) as err:
        lib.host_srs_update(t, n, world["y"])
    assert (err.value.report.bad_points, err.value.report.first_bad_point) == (2, 7)


def test_device_ladder_on_the_cpu_under_sanitizers(tmp_path):
    """tests/cpp/test_srs_update_ladder.hip: the kernel's row ladder (split, windows, complete additions, inversion) as a stand-alone host program (own
    main), the host half built with -fsanitize=address,undefined, against a plain double-and-add: ~3900 scalars"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_srs_update_ladder")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wno-unused-function", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(root, "tests", "cpp", "test_srs_update_ladder.hip"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
