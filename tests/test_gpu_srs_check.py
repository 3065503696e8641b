"""bbgpu_srs_check on the GPU (-m gpu): the curve test over the resident rows (k_srs_on_curve), the multipliers (k_srs_check_scalars), A and B as two
device MSM tickets at offsets 0 and 1, the pairing tail on the host.  Every report is compared, field for field and with a and b, with
bbgpu_host_srs_check on the same table and with the expectations of tests/srs_check_cases.py.  Sizes: n = 2 (one pair), 1000 (no window tables),
4096 (window tables), a prefix of a table, and 2^20 + 8 points, where the table keeps two segments and the offset-1 range starts unaligned and spans both."""
import numpy as np
import pytest

from oracle.pyoracle import FQ, aligned_copy
from tests.srs_check_cases import SEED, fields, g2_of, honest, secret_plus_one, tampers, whole

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
FAR = 1 << 62
# launch checks an honest check without LOCATE passes, whatever n below 2^20 and with or without window tables: the curve test, the multipliers, and
# one per device MSM, which checks its chain of launches once
LAUNCH_CHECKS = 4


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def secret(lib, oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gpu_srs_check")
    x = oracle.random_scalars(0xC0FFEE, 1)[0]
    return dict(x=x, g2_x=g2_of(lib, oracle, tmp, x, "x.dat"), g2_x1=g2_of(lib, oracle, tmp, secret_plus_one(oracle, x), "x1.dat"))


@pytest.fixture(scope="module")
def generated(lib, secret):
    """per size: the handle and host copy of bbgpu_srs_generate's table, and the host copy of the table of x^(5 + i) G; made once, never written to"""
    cache = {}

    def get(n):
        if n not in cache:
            h, table = lib.srs_generate(secret["x"], n, want_host_table=True)
            h5, shifted = lib.srs_generate(secret["x"], n, want_host_table=True, first=5)
            lib.srs_release(h5)
            cache[n] = (h, table, shifted)
        return cache[n]
    return get


def both(lib, handle, table, n, g2, locate=True):
    """the GPU report and the host report of one table; they must agree in every field, a and b included"""
    gpu = lib.srs_check(handle, n, g2, SEED, locate=locate)
    host = lib.host_srs_check(table, n, g2, SEED, locate=locate)
    assert whole(gpu) == whole(host), (fields(gpu), fields(host))
    return gpu


@pytest.mark.parametrize("n", [2, 1000, 4096])
def test_honest_table_and_host_parity(lib, secret, generated, n):
    h, table, _ = generated(n)
    assert lib.srs_has_window_tables(h) == (n >= 1024)
    before = lib.memory_stats()["staging_bytes"]
    rep = both(lib, h, table, n, secret["g2_x"])
    assert fields(rep) == honest(n) and rep.ok
    assert lib.memory_stats()["staging_bytes"] >= max(before, 64 + (n - 1) * 32)  # the multipliers live in library staging
    assert whole(both(lib, h, table, n, secret["g2_x"], locate=False)) == whole(rep)
    assert lib.fault_stats()["slots_pending"] == 0


@pytest.mark.parametrize("kind", ["a", "b", "c", "d", "e", "f", "g"])
@pytest.mark.parametrize("n", [2, 1000, 4096])
def test_tampers_and_host_parity(lib, oracle, secret, generated, n, kind):
    """every tamper of srs_check_cases.py, the edited table registered again: the stated report, equal to the host twin's, first_bad_power included"""
    _, table, shifted = generated(n)
    done = 0
    for name, t, g2, want in tampers(oracle, table, n, secret["g2_x"], secret["g2_x1"], shifted):
        if name[0] != kind:
            continue
        t = aligned_copy(t)  # a table of its own: registering the generated table's host copy again would hand back (and then release) its handle
        h = lib.srs_register(t)
        try:
            rep = both(lib, h, t, n, g2)
            assert fields(rep) == want, (name, fields(rep), want)
            assert rep.ok == (kind in ("f", "g")), name
        finally:
            lib.srs_release(h)
        done += 1
    assert done >= 1 or (kind == "c" and n == 2)  # a swap needs three rows
    assert lib.fault_stats()["slots_pending"] == 0


def test_prefix_of_a_table(lib, secret, generated):
    """n smaller than the table checks a prefix: a bad row behind it is not seen, at its end it is"""
    _, table, _ = generated(4096)
    t = aligned_copy(table)
    t[2 * 3000, 4] += np.uint64(1)
    h = lib.srs_register(t)
    try:
        assert fields(both(lib, h, t, 3000, secret["g2_x"])) == honest(3000)
        rep = both(lib, h, t, 3001, secret["g2_x"])
        assert rep.bad_points == 1 and rep.first_bad_point == 3000 and rep.powers_checked == 0
        assert fields(both(lib, h, t, 1, secret["g2_x"])) == honest(1)
    finally:
        lib.srs_release(h)


def test_five_runs_one_report(lib, oracle, secret, generated):
    h, table, _ = generated(4096)
    assert len({repr(whole(lib.srs_check(h, 4096, secret["g2_x"], SEED, locate=True))) for _ in range(5)}) == 1
    t = aligned_copy(table)
    for k in (17, 1500, 4000):  # several workgroups find something: counts and minima must not depend on who arrives first
        t[2 * k, 4] += np.uint64(1)
    t[2 * 2048, 4:8] = oracle.neg(FQ, t[2 * 2048, 4:8])
    hb = lib.srs_register(t)
    try:
        reps = {repr(whole(lib.srs_check(hb, 4096, secret["g2_x"], SEED, locate=True))) for _ in range(5)}
        assert len(reps) == 1
        rep = lib.srs_check(hb, 4096, secret["g2_x"], SEED)
        assert rep.bad_points == 3 and rep.first_bad_point == 17 and rep.powers_checked == 0
    finally:
        lib.srs_release(hb)
    drawn = [lib.srs_check(h, 4096, secret["g2_x"]) for _ in range(2)]
    assert list(drawn[0].seed) != list(drawn[1].seed) and all(fields(r) == honest(4096) for r in drawn)


def test_launch_checks_do_not_depend_on_n(lib, secret, generated):
    """an honest check without LOCATE passes a fixed number of launch checks (and, warm, no allocation, one upload and one read-back through the funnels)"""
    seen = {}
    for n in (1000, 4096):
        h, _, _ = generated(n)
        assert lib.srs_check(h, n, secret["g2_x"], SEED).ok  # warm
        lib.fault_inject("launch:%d" % FAR)
        assert lib.srs_check(h, n, secret["g2_x"], SEED).ok
        seen[n] = lib.fault_stats()
        lib.fault_inject(None)
    print("launch checks per honest check:", {n: st["launch_checks"] for n, st in seen.items()})
    for n, st in seen.items():
        assert (st["alloc_calls"], st["h2d_calls"], st["d2h_calls"]) == (0, 1, 1), (n, st)
    assert len({st["launch_checks"] for st in seen.values()}) == 1, seen
    assert seen[4096]["launch_checks"] == LAUNCH_CHECKS, seen


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, secret, generated, kind):
    """every site of the funnel `kind` that one warm check at n = 4096 passes, failed once: an error return, no MSM slot pending, the live allocations of
    before the call, and the very next check correct"""
    from barretenberg_amd import BbGpuError
    n = 4096
    h, table, _ = generated(n)
    want = whole(lib.srs_check(h, n, secret["g2_x"], SEED))  # warm
    assert want["ok"]
    lib.fault_inject("%s:%d" % (kind, FAR))
    assert whole(lib.srs_check(h, n, secret["g2_x"], SEED)) == want
    st = lib.fault_stats()
    sites = {"alloc": st["alloc_calls"], "h2d": st["h2d_calls"], "d2h": st["d2h_calls"], "launch": st["launch_checks"]}[kind]
    live = st["live_allocations"]
    assert sites >= {"alloc": 0, "h2d": 1, "d2h": 1, "launch": 4}[kind], st
    for k in range(sites):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError):
            lib.srs_check(h, n, secret["g2_x"], SEED)
        st = lib.fault_stats()
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["slots_pending"] == 0 and st["live_allocations"] == live, (kind, k, st)
        assert whole(lib.srs_check(h, n, secret["g2_x"], SEED)) == want, (kind, k)
    lib.fault_inject(None)


def test_across_the_segment_boundary(lib, oracle, secret):
    """2^20 + 8 points: the table keeps two segments, the offset-1 range starts unaligned and spans both.  GPU verdict only."""
    n = (1 << 20) + 8
    h, table = lib.srs_generate(secret["x"], n, want_host_table=True)
    try:
        assert lib.srs_has_window_tables(h)
        assert fields(lib.srs_check(h, n, secret["g2_x"], SEED, locate=True)) == honest(n)
    finally:
        lib.srs_release(h)
    k = 1 << 20
    table[2 * k, 4:8] = oracle.neg(FQ, table[2 * k, 4:8])
    h = lib.srs_register(table)
    try:
        rep = lib.srs_check(h, n, secret["g2_x"], SEED, locate=True)
        assert fields(rep) == dict(honest(n), powers_ok=0, first_bad_power=k - 1), fields(rep)
    finally:
        lib.srs_release(h)
    assert lib.fault_stats()["slots_pending"] == 0


def test_argument_errors_on_a_bound_device(lib, secret, generated):
    from barretenberg_amd import BbGpuError
    h, _, _ = generated(1000)
    for bad in (lambda: lib.srs_check(h, 0), lambda: lib.srs_check(h, 1001), lambda: lib.srs_check(1 << 20, 10)):
        with pytest.raises(BbGpuError, match=" -3:"):
            bad()
    assert lib.srs_check(h, 1000).ok  # no x * G2: the curve test decides
