"""bbgpu_srs_update on the GPU (-m gpu): the curve pass over the input rows, k_srs_update (csrc/srs_update.hip: the endomorphism split and one ladder over
both halves per lane), the export kernel, the registration of the new table.  Every exported table is compared bit for bit with the oracle's
(tests/srs_update_cases.py) and with bbgpu_host_srs_update's, and the two reports field for field.  Sizes: n = 1 (one lane), 2 (one pair), 300 (the bit walk
with y = 2; a partial wave and a partial workgroup), 1000 (no window tables on the new handle), 4096 (window tables)."""
import numpy as np
import pytest

from oracle.pyoracle import FR, aligned_copy, from_int
from tests.srs_check_cases import SEED, g2_of
from tests.srs_update_cases import (NONE, all_g_table, check_split, honest_table, mont, row_times, row_times_plain, rows_times_powers, secret_x, secret_y,
                                    special_ys, split_cases, tampered, unrelated_points, updated_table)

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 300, 1000, 4096]
KINDS = ("alloc", "h2d", "d2h", "launch")
FAR = 1 << 62
# the funnels one warm honest update of 4096 rows passes: allocations -- the new rows, the export buffer, the window tables of one segment;
# uploads -- the curve findings' start value; read-backs -- the findings, the host table (512 KiB: one staging chunk); launch checks -- the curve pass,
# k_srs_update, the export kernel, the window tables
WARM_4096 = dict(alloc_calls=3, h2d_calls=1, d2h_calls=2, launch_checks=4)
WARM_4096_RESIDENT_ONLY = dict(alloc_calls=2, h2d_calls=1, d2h_calls=1, launch_checks=3)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def world(lib, oracle, tmp_path_factory):
    """the secrets, the generated table of x (handle and host copy) and the oracle's update of it by y at the largest size, x G2 and (x y) G2: made once,
    never written to"""
    tmp = tmp_path_factory.mktemp("gpu_srs_update")
    x, y = secret_x(oracle), secret_y(oracle)
    xy = oracle.mul(FR, x, y)
    h, table = lib.srs_generate(x, 4096, want_host_table=True)
    assert np.array_equal(table, honest_table(oracle, x, 4096))
    return dict(x=x, y=y, xy=xy, h=h, table=table, want=updated_table(oracle, x, y, 4096), g2_x=g2_of(lib, oracle, tmp, x, "x.dat"),
                g2_xy=g2_of(lib, oracle, tmp, xy, "xy.dat"))


def whole(rep):
    return rep.as_dict()


def test_split_on_the_device(lib, oracle, golden):
    """the split as the kernel computes it (64-bit integer C++, __umul64hi): the golden values of tests/golden/endo_wnaf.json, a split of every other scalar"""
    pinned, free = split_cases(oracle, golden)
    ks = np.array([from_int(k) for k, _, _ in pinned] + [from_int(k) for k in free], dtype=np.uint64)
    out = lib.selftest_endo_split(ks, on_device=True)
    check_split(oracle, pinned, free, out)
    assert np.array_equal(out, lib.selftest_endo_split(ks, on_device=False))


@pytest.mark.parametrize("n", SIZES)
def test_oracle_and_host_parity(lib, oracle, world, n):
    live = lib.srs_cache_stats()[0]
    h, table, rep = lib.srs_update(world["h"], n, world["y"], world["g2_x"], want_host_table=True)
    try:
        assert np.array_equal(table, world["want"][:2 * n])
        host, host_rep = lib.host_srs_update(aligned_copy(world["table"][:2 * n]), n, world["y"], world["g2_x"])
        assert np.array_equal(table, host)
        assert whole(rep) == whole(host_rep)
        assert (rep.n, rep.first_power, rep.bad_points, rep.first_bad_point, rep.g2_ok) == (n, 0, 0, NONE, 1)
        assert np.array_equal(np.array(rep.g2_x_out, dtype=np.uint64), world["g2_xy"])
        assert lib.srs_has_window_tables(h) == (n >= 1024)
        assert lib.srs_cache_stats()[0] == live + 1
    finally:
        lib.srs_release(h)
    assert lib.fault_stats()["slots_pending"] == 0


def test_bit_walk(lib, oracle, world):
    """y = 2 over 300 rows: the set bit of the scalar walks through every window boundary of both halves, and from row 254 on the power wraps modulo r"""
    two = mont(oracle, 2)
    h, table, _ = lib.srs_update(world["h"], 300, two, want_host_table=True)
    lib.srs_release(h)
    assert np.array_equal(table, updated_table(oracle, world["x"], two, 300))


def test_special_scalars_on_single_rows(lib, oracle):
    """n = 1, first_power = 1, a row that is not the generator, one call per scalar"""
    p = unrelated_points(oracle, 3)[1:2]
    h0 = lib.srs_register(oracle.point_table(aligned_copy(p)))
    try:
        for name, y in special_ys(oracle):
            h, table, rep = lib.srs_update(h0, 1, y, want_host_table=True, first=1)
            lib.srs_release(h)
            assert np.array_equal(table[0], row_times_plain(oracle, p[0], y)), name
            assert name == "negative-t" or np.array_equal(table[0], row_times(oracle, p[0], y)), name
            assert rep.first_power == 1 and rep.n == 1
    finally:
        lib.srs_release(h0)


def test_special_scalars_in_one_wave(lib, oracle):
    """the same scalars side by side in the lanes of one wave: y^(1 + i) for every special y over unrelated rows, divergent exceptional cases included"""
    pts = unrelated_points(oracle, 7)
    h0 = lib.srs_register(oracle.point_table(pts))
    try:
        for name, y in special_ys(oracle):
            h, table, _ = lib.srs_update(h0, 7, y, want_host_table=True, first=1)
            lib.srs_release(h)
            host, _ = lib.host_srs_update(oracle.point_table(pts), 7, y, first=1)
            assert np.array_equal(table, host), name
            if name in ("random", "two", "r-1", "lambda"):
                assert np.array_equal(table, rows_times_powers(oracle, pts, y, first=1)), name
    finally:
        lib.srs_release(h0)


def test_all_g_table(lib, oracle, world):
    n = 300
    h0 = lib.srs_register(all_g_table(oracle, n))
    try:
        h, table, _ = lib.srs_update(h0, n, world["y"], want_host_table=True)
        lib.srs_release(h)
        assert np.array_equal(table, honest_table(oracle, world["y"], n))
    finally:
        lib.srs_release(h0)


def test_new_handle(lib, oracle, world):
    """the new handle serves MSMs, passes the check with its own x G2 and fails it with the old one; the input handle is untouched"""
    import torch
    n = 4096
    h, table, rep = lib.srs_update(world["h"], n, world["y"], world["g2_x"], want_host_table=True)
    try:
        g2_out = np.array(rep.g2_x_out, dtype=np.uint64)
        sc = oracle.random_scalars(0xA11CE, n)
        d = torch.from_numpy(sc.view(np.int64)).cuda()
        assert lib.srs_has_window_tables(h)
        assert np.array_equal(lib.msm_device(h, d.data_ptr(), n)[:8], oracle.msm_affine(sc, table, n)[:8])
        assert np.array_equal(lib.pippenger(sc, table, n)[:8], oracle.msm_affine(sc, table, n)[:8])  # the host table is the address key of the new handle
        assert lib.srs_check(h, n, g2_out, SEED).ok
        old = lib.srs_check(h, n, world["g2_x"], SEED)
        assert old.powers_checked == 1 and old.powers_ok == 0
        assert lib.srs_check(world["h"], n, world["g2_x"], SEED).ok
        assert lib.host_srs_update_check(world["table"][2], table[2], np.array(rep.y_g2, dtype=np.uint64))
        # resident only: no host table, the same rows (an MSM over them tells)
        h2, none, rep2 = lib.srs_update(world["h"], n, world["y"], world["g2_x"])
        assert none is None and whole(rep2) == whole(rep)
        assert np.array_equal(lib.msm_device(h2, d.data_ptr(), n)[:8], oracle.msm_affine(sc, table, n)[:8])
        lib.srs_release(h2)
        # bbgpu_set_precompute is honoured
        lib.set_precompute(False)
        try:
            h3, _, _ = lib.srs_update(world["h"], n, world["y"])
            assert not lib.srs_has_window_tables(h3)
            assert np.array_equal(lib.msm_device(h3, d.data_ptr(), n)[:8], oracle.msm_affine(sc, table, n)[:8])
            lib.srs_release(h3)
        finally:
            lib.set_precompute(True)
    finally:
        lib.srs_release(h)
    assert lib.fault_stats()["slots_pending"] == 0


def test_prefix_and_offset(lib, oracle, world):
    h, table, rep = lib.srs_update(world["h"], 3000, world["y"], want_host_table=True)
    lib.srs_release(h)
    assert rep.n == 3000 and np.array_equal(table, world["want"][:6000])
    n = 300
    h5, shifted = lib.srs_generate(world["x"], n, want_host_table=True, first=5)
    try:
        assert np.array_equal(shifted, world["table"][10:2 * (n + 5)])
        h, table, rep = lib.srs_update(h5, n, world["y"], world["g2_x"], want_host_table=True, first=5)
        lib.srs_release(h)
        assert np.array_equal(table, world["want"][10:2 * (n + 5)]) and rep.first_power == 5
        assert np.array_equal(np.array(rep.g2_x_out, dtype=np.uint64), world["g2_xy"])  # only the first power enters G2
    finally:
        lib.srs_release(h5)


def test_five_runs_one_table(lib, world):
    tables = []
    for _ in range(5):
        h, table, _ = lib.srs_update(world["h"], 4096, world["y"], want_host_table=True)
        lib.srs_release(h)
        tables.append(table)
    assert all(np.array_equal(t, tables[0]) for t in tables) and np.array_equal(tables[0], world["want"])


def test_bad_rows(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    n = 4096
    for k in (0, n // 2, n - 1):
        t = tampered(world["table"], k)
        hb = lib.srs_register(t)
        try:
            live = lib.srs_cache_stats()[0]
            allocations = lib.fault_stats()["live_allocations"]
            with pytest.raises(BbGpuError, match=" -3:.*row %d " % k) as err:
                lib.srs_update(hb, n, world["y"], world["g2_x"], want_host_table=True)
            rep = err.value.report
            assert (rep.n, rep.bad_points, rep.first_bad_point, rep.g2_ok) == (n, 1, k, 1)
            with pytest.raises(BbGpuError) as host_err:
                lib.host_srs_update(t, n, world["y"], world["g2_x"])
            assert whole(host_err.value.report) == whole(rep)
            assert lib.srs_cache_stats()[0] == live and lib.fault_stats()["live_allocations"] == allocations
            if k:  # a prefix that ends before the bad row is updated
                h, table, _ = lib.srs_update(hb, k, world["y"], want_host_table=True)
                lib.srs_release(h)
                assert np.array_equal(table, world["want"][:2 * k])
        finally:
            lib.srs_release(hb)


def test_argument_errors(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    from oracle.pyoracle import FR_MODULUS
    live = lib.srs_cache_stats()[0]
    h, y = world["h"], world["y"]
    for bad in (lambda: lib.srs_update(h, 0, y), lambda: lib.srs_update(h, 4097, y), lambda: lib.srs_update(1 << 20, 10, y), lambda: lib.srs_update(h, 10, None),
                lambda: lib.srs_update(h, 10, np.zeros(4, dtype=np.uint64)), lambda: lib.srs_update(h, 10, from_int(FR_MODULUS)),
                lambda: lib.srs_update(h, 10, y, first=(1 << 32) - 9)):
        with pytest.raises(BbGpuError, match=" -3:"):
            bad()
    assert lib.srs_cache_stats()[0] == live


def test_funnel_counts_of_a_warm_update(lib, world):
    n = 4096
    for want_table, want in ((True, WARM_4096), (False, WARM_4096_RESIDENT_ONLY)):
        h, _, _ = lib.srs_update(world["h"], n, world["y"], want_host_table=want_table)  # warm
        lib.srs_release(h)
        lib.fault_inject("launch:%d" % FAR)
        h, _, _ = lib.srs_update(world["h"], n, world["y"], want_host_table=want_table)
        st = lib.fault_stats()
        lib.fault_inject(None)
        lib.srs_release(h)
        print("funnels of one warm update of %d rows, host table %s:" % (n, want_table), {k: st[k] for k in want})
        assert {k: st[k] for k in want} == want, st


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, world, kind):
    """every site of the funnel `kind` that one warm update of 4096 rows passes, failed once.  These are host-side funnels; nothing faults on the device.
    A fired failure returns an error and creates no handle -- except in the window tables of the NEW handle, which bbgpu_srs_update builds through the
    add_srs path of bbgpu_srs_generate_range: there the library rides the failure out (counted as absorbed) and the handle serves without tables, with the
    right rows.  Either way the live allocations are those of before once the handle is gone, no MSM slot is pending, and the next call is right."""
    from barretenberg_amd import BbGpuError
    n = 4096
    h, table, _ = lib.srs_update(world["h"], n, world["y"], want_host_table=True)  # warm
    lib.srs_release(h)
    assert np.array_equal(table, world["want"])
    before = lib.fault_stats()
    entries = lib.srs_cache_stats()[0]
    lib.fault_inject("%s:%d" % (kind, FAR))
    h, _, _ = lib.srs_update(world["h"], n, world["y"], want_host_table=True)
    st = lib.fault_stats()
    lib.srs_release(h)
    sites = {"alloc": st["alloc_calls"], "h2d": st["h2d_calls"], "d2h": st["d2h_calls"], "launch": st["launch_checks"]}[kind]
    assert sites == WARM_4096[{"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}[kind]], st
    absorbed = 0
    for k in range(sites + 1):  # k == sites: the armed failure no longer fires
        lib.fault_inject("%s:%d" % (kind, k))
        try:
            h, table, _ = lib.srs_update(world["h"], n, world["y"], want_host_table=True)
        except BbGpuError:
            st = lib.fault_stats()
            assert k < sites and st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
            assert lib.srs_cache_stats()[0] == entries, (kind, k)
        else:
            st = lib.fault_stats()
            if k < sites:  # ridden out: the window tables of the new handle
                assert st["fired"] == 1 and st["absorbed"] == 1 and not lib.srs_has_window_tables(h), (kind, k, st)
                absorbed += 1
            else:
                assert st["fired"] == 0 and st["armed"] == 1 and lib.srs_has_window_tables(h), (kind, k, st)
            assert np.array_equal(table, world["want"]), (kind, k)
            lib.srs_release(h)
        lib.fault_inject(None)
        st = lib.fault_stats()
        assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        h, table, _ = lib.srs_update(world["h"], n, world["y"], want_host_table=True)
        lib.srs_release(h)
        assert np.array_equal(table, world["want"]), (kind, k)
    assert absorbed == (1 if kind in ("alloc", "launch") else 0)  # the tables' allocation, the tables' launch check
