"""bbgpu_srs_lagrange on the GPU (-m gpu): the curve pass over the input rows, the kernels of csrc/srs_lagrange.hip (the scaled bit-reversed load, one
butterfly per lane and stage on projective points, the normalisation that counts infinities), the export kernel, the registration of the new table.  Every
exported table is compared bit for bit with bbgpu_host_srs_lagrange's -- itself held to the definition by tests/test_srs_lagrange_host.py -- and the two
reports field for field.  Sizes: n = 2 (one butterfly), 4, 8 (a partial wave), 64, 128 (exactly one wave of butterflies), 256 (two workgroups), 1024 (the
first size with window tables), 4096 (twelve stages); 2^14 and 2^20 (past the grid of the finish kernel) through the MSM identity only."""
import numpy as np
import pytest

from oracle.pyoracle import aligned_copy
from tests.srs_lagrange_cases import (NONE, all_g_table, collision_table, honest_table, omega_table, secret_x, tampered)

pytestmark = pytest.mark.gpu
SIZES = [2, 4, 8, 64, 128, 256, 1024, 4096]
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
# the funnels one warm honest conversion passes.  256 rows: allocations -- the scratch, the new rows, the export buffer; uploads -- the start
# value of both findings; read-backs -- the curve findings, the infinity findings, the host table (one staging chunk); launch checks -- the curve pass, the
# chain of load, stage and finish kernels, the export kernel.  1024 rows: the window tables of one segment add an allocation and a launch check.
WARM = {(256, True): dict(alloc_calls=3, h2d_calls=1, d2h_calls=3, launch_checks=3), (256, False): dict(alloc_calls=2, h2d_calls=1, d2h_calls=2, launch_checks=2),
        (1024, True): dict(alloc_calls=4, h2d_calls=1, d2h_calls=3, launch_checks=4), (1024, False): dict(alloc_calls=3, h2d_calls=1, d2h_calls=2, launch_checks=3)}
BIG = 1 << 14
HUGE = 1 << 20  # k_lagrange_finish runs 2048 workgroups of 256: rows from 2^19 on are a thread's second


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def world(lib, oracle):
    """the generated table of a known x (handle and host copy) and, per size, the host twin's conversion of its first rows: made once, never written to"""
    h, table = lib.srs_generate(secret_x(oracle), BIG, want_host_table=True)
    assert np.array_equal(table[:2 * 4096], honest_table(oracle, secret_x(oracle), 4096))
    made = {}

    def host(n):
        if n not in made:
            made[n] = lib.host_srs_lagrange(aligned_copy(table[:2 * n]), n)
        return made[n]
    return dict(h=h, table=table, host=host)


def whole(rep):
    return rep.as_dict()


@pytest.mark.parametrize("n", SIZES)
def test_host_parity(lib, world, n):
    live = lib.srs_cache_stats()[0]
    h, table, rep = lib.srs_lagrange(world["h"], n, want_host_table=True)
    try:
        host, host_rep = world["host"](n)
        assert np.array_equal(table, host)
        assert whole(rep) == whole(host_rep)
        assert whole(rep) == dict(n=n, bad_points=0, first_bad_point=NONE, infinity_rows=0, first_infinity_row=NONE)
        assert lib.srs_has_window_tables(h) == (n >= 1024)
        assert lib.srs_cache_stats()[0] == live + 1
    finally:
        lib.srs_release(h)
    assert lib.fault_stats()["slots_pending"] == 0


@pytest.mark.parametrize("n", [4096, BIG, HUGE])
def test_the_handle_commits_to_values(lib, oracle, world, n):
    """sum_i v_i L_i over the new handle == sum_j ifft(v)_j P_j over the input handle, both by the device MSM; the input handle is untouched.  Random v
    make every output row count: at 2^20 rows (an input handle of its own) that includes the rows the finish kernel writes in its second trip."""
    import torch
    source = world["h"] if n <= BIG else lib.srs_generate(secret_x(oracle), n)
    try:
        v = oracle.random_scalars(0x7A61 + n, n)
        c = lib.ntt(aligned_copy(v), "ifft")
        dv, dc = torch.from_numpy(v.view(np.int64)).cuda(), torch.from_numpy(c.view(np.int64)).cuda()
        h, table, rep = lib.srs_lagrange(source, n, want_host_table=(n == 4096))
        try:
            assert whole(rep) == dict(n=n, bad_points=0, first_bad_point=NONE, infinity_rows=0, first_infinity_row=NONE)
            assert lib.srs_has_window_tables(h)
            got = lib.msm_device(h, dv.data_ptr(), n)[:8]
            assert np.array_equal(got, lib.msm_device(source, dc.data_ptr(), n)[:8])
            if n == 4096:
                assert np.array_equal(got, oracle.msm_affine(v, aligned_copy(table), n)[:8])
                assert np.array_equal(lib.pippenger(v, table, n)[:8], got)  # the host table is the address key of the new handle
        finally:
            lib.srs_release(h)
    finally:
        if n > BIG:
            lib.srs_release(source)
    assert lib.fault_stats()["slots_pending"] == 0


def test_the_string_of_the_secret_one_at_two_to_the_twenty(lib, oracle):
    """P_0 .. P_(n-1) all G (generated under the secret 1): every output row but row 0 is at infinity.  The refusal's report is the sum of the counts of
    both trips of the finish kernel's 2^19 threads, and a minimum that lives in the first"""
    from barretenberg_amd import BbGpuError
    from oracle.pyoracle import FR
    h0 = lib.srs_generate(oracle.const(FR, "one"), HUGE)
    try:
        live, allocations = lib.srs_cache_stats()[0], lib.fault_stats()["live_allocations"]
        with pytest.raises(BbGpuError, match=" -3:.*row 1 ") as err:
            lib.srs_lagrange(h0, HUGE)
        assert whole(err.value.report) == dict(n=HUGE, bad_points=0, first_bad_point=NONE, infinity_rows=HUGE - 1, first_infinity_row=1)
        assert lib.srs_cache_stats()[0] == live and lib.fault_stats()["live_allocations"] == allocations
    finally:
        lib.srs_release(h0)


def special_tables(oracle, honest):
    """(name, n, table): the degenerate and collision tables of tests/test_srs_lagrange_host.py, and their like at 64 rows (one wave: the exceptional cases
    sit in lanes beside ordinary ones)"""
    return [("x = 1", 8, all_g_table(oracle, 8)), ("x = omega^3", 16, omega_table(oracle, 16, 3)), ("x = omega^5", 64, omega_table(oracle, 64, 5)),
            ("x = 1", 64, all_g_table(oracle, 64)), ("off the curve", 64, tampered(honest[:128], 37)), ("off the curve", 8, tampered(honest[:16], 0)),
            ("collisions", 8, collision_table(oracle, 8, 1, 2)), ("collisions", 16, collision_table(oracle, 16, 0, 7)),
            ("collisions", 64, collision_table(oracle, 64, 3, 17))]


def test_degenerate_and_collision_tables(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    refusals = 0
    for name, n, t in special_tables(oracle, world["table"]):
        h0 = lib.srs_register(t)
        try:
            live, allocations = lib.srs_cache_stats()[0], lib.fault_stats()["live_allocations"]
            try:
                host, host_rep = lib.host_srs_lagrange(t, n)
            except BbGpuError as e:
                host, host_rep = None, e.report
            if host is None:
                with pytest.raises(BbGpuError, match=" -3:.*row %d " % (host_rep.first_bad_point if host_rep.bad_points else host_rep.first_infinity_row)) as err:
                    lib.srs_lagrange(h0, n, want_host_table=True)
                assert whole(err.value.report) == whole(host_rep), (name, n)
                assert lib.srs_cache_stats()[0] == live and lib.fault_stats()["live_allocations"] == allocations, (name, n)
                refusals += 1
            else:
                h, table, rep = lib.srs_lagrange(h0, n, want_host_table=True)
                lib.srs_release(h)
                assert np.array_equal(table, host), (name, n)
                assert whole(rep) == whole(host_rep), (name, n)
        finally:
            lib.srs_release(h0)
    assert refusals == 6  # the collision tables convert: every output row is finite
    assert lib.fault_stats()["slots_pending"] == 0


def test_argument_errors(lib, world):
    from barretenberg_amd import BbGpuError
    live = lib.srs_cache_stats()[0]
    h = world["h"]
    for n, handle, code in ((0, h, " -3:"), (64, 1 << 20, " -3:"), (1, h, " -2:"), (3, h, " -2:"), (1 << 23, h, " -2:"), (2 * BIG, h, " -2:")):
        with pytest.raises(BbGpuError, match=code):
            lib.srs_lagrange(handle, n)
    assert lib.srs_cache_stats()[0] == live


@pytest.mark.parametrize("n", [256, 1024])
def test_funnel_counts_of_a_warm_call(lib, world, n):
    for want_table in (True, False):
        h, _, _ = lib.srs_lagrange(world["h"], n, want_host_table=want_table)  # warm
        lib.srs_release(h)
        lib.fault_inject("launch:%d" % FAR)
        h, _, _ = lib.srs_lagrange(world["h"], n, want_host_table=want_table)
        st = lib.fault_stats()
        lib.fault_inject(None)
        lib.srs_release(h)
        want = WARM[(n, want_table)]
        print("funnels of one warm conversion of %d rows, host table %s:" % (n, want_table), {k: st[k] for k in want})
        assert {k: st[k] for k in want} == want, st


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, world, kind):
    """every site of the funnel `kind` that one warm conversion of 1024 rows passes, failed once.  These are host-side funnels; nothing faults on the
    device.  A fired failure returns an error and creates no handle -- except in the window tables of the NEW handle, built through add_srs: there the
    library rides the failure out (counted as absorbed) and the handle serves without tables, with the right rows.  Either way the live allocations are those
    of before once the handle is gone, no MSM slot is pending, and the next call is right."""
    from barretenberg_amd import BbGpuError
    n = 1024
    want, _ = world["host"](n)
    h, table, _ = lib.srs_lagrange(world["h"], n, want_host_table=True)  # warm
    lib.srs_release(h)
    assert np.array_equal(table, want)
    before = lib.fault_stats()
    entries = lib.srs_cache_stats()[0]
    sites = WARM[(n, True)][KEYS[kind]]
    absorbed = 0
    for k in range(sites + 1):  # k == sites: the armed failure no longer fires
        lib.fault_inject("%s:%d" % (kind, k))
        try:
            h, table, _ = lib.srs_lagrange(world["h"], n, want_host_table=True)
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
            assert np.array_equal(table, want), (kind, k)
            lib.srs_release(h)
        lib.fault_inject(None)
        st = lib.fault_stats()
        assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        h, table, _ = lib.srs_lagrange(world["h"], n, want_host_table=True)
        lib.srs_release(h)
        assert np.array_equal(table, want), (kind, k)
    assert absorbed == (1 if kind in ("alloc", "launch") else 0)  # the tables' allocation, the tables' launch check


def test_stage_kernel_time_is_reported(lib, world):
    lib.set_timing(1)
    try:
        h, _, _ = lib.srs_lagrange(world["h"], 4096)
        lib.srs_release(h)
        ms = lib.last_timing()
    finally:
        lib.set_timing(0)
    assert len(ms) == 3 and all(0 < v < 1000 for v in ms), ms  # the stage kernels, the load kernel, the finish kernel
