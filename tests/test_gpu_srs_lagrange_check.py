"""bbgpu_srs_lagrange_check on the GPU (-m gpu): the curve pass over the Lagrange rows, the multipliers, their transformed copy, A and B as two device MSM
tickets, the verdict and its bisection on the host.  Every report is compared, field for field and with a and b, with bbgpu_host_srs_lagrange_check on the
same tables -- itself pinned by tests/test_srs_lagrange_check_host.py.  Sizes: n = 2 (one butterfly), 64 (no window tables), 1024 (the first size with
window tables), 4096 (a transform of two passes); 2^16 for the honest verdict alone.  Tampered rows sit at 0, 63, 64 (the last lane of a wave and the first
of the next in the curve pass), n / 2 and n - 1."""
import numpy as np
import pytest

from oracle.pyoracle import FQ, aligned_copy
from tests.srs_check_cases import SEED
from tests.srs_lagrange_cases import ERR_ARG, ERR_SIZE, NONE, secret_x, tampered

pytestmark = pytest.mark.gpu
SIZES = [2, 64, 1024, 4096]
BIG = 1 << 16
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
# the funnels one warm honest check of 4096 rows without LOCATE passes: no allocation; one upload, the start value of the findings; one
# read-back, the findings; launch checks -- the curve pass, the multipliers, the two passes of the 4096-point transform, and one per device MSM, which
# checks its chain of launches once
WARM = dict(alloc_calls=0, h2d_calls=1, d2h_calls=1, launch_checks=6)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def world(lib, oracle):
    """the generated string of a known x (handle and host copy) and, per size, the Lagrange handle of its first rows with its exported table: made once,
    never written to"""
    h, table = lib.srs_generate(secret_x(oracle), BIG, want_host_table=True)
    made = {}

    def lagrange(n):
        if n not in made:
            hl, t, _ = lib.srs_lagrange(h, n, want_host_table=(n < BIG))
            made[n] = (hl, t)
        return made[n]
    return dict(h=h, table=table, lagrange=lagrange)


def whole(rep):
    return rep.as_dict()


def verdict(rep):
    return (rep.n, rep.bad_points, rep.first_bad_point, rep.basis_checked, rep.basis_ok, rep.first_bad_row)


def both(lib, world, hl, lag_table, n, locate=True):
    gpu = lib.srs_lagrange_check(hl, world["h"], n, seed=SEED, locate=locate)
    host = lib.host_srs_lagrange_check(lag_table, world["table"][:2 * n], n=n, seed=SEED, locate=locate)
    assert whole(gpu) == whole(host), (verdict(gpu), verdict(host))
    return gpu


@pytest.mark.parametrize("n", SIZES)
def test_honest_table_and_host_parity(lib, world, n):
    hl, t = world["lagrange"](n)
    assert lib.srs_has_window_tables(hl) == (n >= 1024)
    rep = both(lib, world, hl, t, n)
    assert verdict(rep) == (n, 0, NONE, 1, 1, NONE) and rep.ok and list(rep.seed) == [int(v) for v in SEED]
    assert np.array_equal(np.array(rep.a), np.array(rep.b))
    assert whole(both(lib, world, hl, t, n, locate=False)) == whole(rep)
    assert lib.fault_stats()["slots_pending"] == 0


def test_honest_table_of_65536_rows(lib, world):
    hl, _ = world["lagrange"](BIG)
    rep = lib.srs_lagrange_check(hl, world["h"], BIG, seed=SEED, locate=True)
    assert verdict(rep) == (BIG, 0, NONE, 1, 1, NONE)
    drawn = lib.srs_lagrange_check(hl, world["h"], BIG)  # NULL seed: drawn, reported, replayable
    assert drawn.ok and any(drawn.seed) and list(drawn.seed) != list(rep.seed)
    assert whole(lib.srs_lagrange_check(hl, world["h"], BIG, seed=np.array(list(drawn.seed), dtype=np.uint64))) == whole(drawn)


def test_an_exported_table_registered_again_passes(lib, world):
    """the use the entry exists for: the table leaves the process and comes back through bbgpu_srs_register"""
    n = 1024
    _, t = world["lagrange"](n)
    back = aligned_copy(t)
    h2 = lib.srs_register(back)
    try:
        assert whole(lib.srs_lagrange_check(h2, world["h"], n, seed=SEED)) == whole(lib.srs_lagrange_check(world["lagrange"](n)[0], world["h"], n, seed=SEED))
        assert lib.srs_lagrange_check(h2, world["h"], n, seed=SEED).ok
    finally:
        lib.srs_release(h2)


@pytest.mark.parametrize("n", [64, 1024, 4096])
def test_tampered_rows_are_located(lib, oracle, world, n):
    """one row replaced by another point of the curve, the edited table registered again; the host twin's report for it up to 1024 rows"""
    _, t = world["lagrange"](n)
    for k in sorted({0, 63, 64, n // 2, n - 1} & set(range(n))):
        bad = aligned_copy(t)
        bad[2 * k:2 * k + 2] = t[2 * ((k + 7) % n):2 * ((k + 7) % n) + 2]
        hb = lib.srs_register(bad)
        try:
            rep = both(lib, world, hb, bad, n) if n <= 1024 else lib.srs_lagrange_check(hb, world["h"], n, seed=SEED, locate=True)
            assert verdict(rep) == (n, 0, NONE, 1, 0, k), k
            assert verdict(lib.srs_lagrange_check(hb, world["h"], n, seed=SEED)) == (n, 0, NONE, 1, 0, NONE), k
        finally:
            lib.srs_release(hb)
    bad = aligned_copy(t)  # a negated row and, behind it, two rows exchanged: the smallest index
    bad[2 * 5, 4:8] = oracle.neg(FQ, bad[2 * 5, 4:8])
    bad[[2 * 9, 2 * 9 + 1, 2 * 40, 2 * 40 + 1]] = bad[[2 * 40, 2 * 40 + 1, 2 * 9, 2 * 9 + 1]]
    hb = lib.srs_register(bad)
    try:
        assert verdict(lib.srs_lagrange_check(hb, world["h"], n, seed=SEED, locate=True)) == (n, 0, NONE, 1, 0, 5)
    finally:
        lib.srs_release(hb)
    assert lib.fault_stats()["slots_pending"] == 0


def test_an_off_curve_row_stops_the_check(lib, world):
    n = 1024
    _, t = world["lagrange"](n)
    bad = tampered(tampered(t, 700), 63)
    hb = lib.srs_register(bad)
    try:
        rep = both(lib, world, hb, bad, n)
        assert verdict(rep) == (n, 2, 63, 0, 0, NONE) and not rep.ok and rep.a[7] == 1 << 63 and rep.b[7] == 1 << 63
    finally:
        lib.srs_release(hb)


def test_handles_of_different_sizes_and_argument_errors(lib, world):
    from barretenberg_amd import BbGpuError
    h = world["h"]
    hl64, t64 = world["lagrange"](64)
    hl1024, _ = world["lagrange"](1024)
    assert lib.srs_lagrange_check(hl64, h, 64, seed=SEED).ok  # 64 rows against the first 64 of 65536
    assert verdict(lib.srs_lagrange_check(hl1024, h, 64, seed=SEED))[3:5] == (1, 0)  # the first 64 of 1024 Lagrange rows are no Lagrange form of 64
    live = lib.fault_stats()["live_allocations"]
    for args, code in (((hl64, h, 128), ERR_SIZE), ((hl64, h, 0), ERR_SIZE), ((hl64, h, 48), ERR_SIZE), ((hl64, h, 1 << 23), ERR_SIZE),
                       ((1 << 20, h, 64), ERR_ARG), ((hl64, -1, 64), ERR_ARG), ((hl64, 1 << 20, 64), ERR_ARG)):
        with pytest.raises(BbGpuError, match=code):
            lib.srs_lagrange_check(*args, seed=SEED)
    import ctypes as C
    from barretenberg_amd.bbgpu import SrsLagrangeCheckReport
    rep = SrsLagrangeCheckReport()
    assert lib.lib.bbgpu_srs_lagrange_check(hl64, h, 64, None, 0, None) == -3
    assert lib.lib.bbgpu_srs_lagrange_check(hl64, h, 64, None, 2, C.byref(rep)) == -3
    assert lib.fault_stats()["live_allocations"] == live and lib.fault_stats()["slots_pending"] == 0


def test_the_handles_are_untouched(lib, oracle, world):
    """the MSMs of both handles over a fixed scalar vector return the same points after checks, a located failure included"""
    import torch
    n = 4096
    hl, t = world["lagrange"](n)
    d_s = torch.from_numpy(oracle.random_scalars(0x5CA1A, n).view(np.int64)).cuda()
    before = (lib.msm_device(hl, d_s.data_ptr(), n), lib.msm_device(world["h"], d_s.data_ptr(), n))
    assert lib.srs_lagrange_check(hl, world["h"], n, seed=SEED, locate=True).ok
    assert not lib.srs_lagrange_check(world["h"], world["h"], n, seed=SEED, locate=True).ok  # a string is not its own Lagrange form: bisected
    after = (lib.msm_device(hl, d_s.data_ptr(), n), lib.msm_device(world["h"], d_s.data_ptr(), n))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[0], lib.pippenger(aligned_copy(oracle.random_scalars(0x5CA1A, n)), t, n))


def test_funnel_counts_of_a_warm_call(lib, world):
    n = 4096
    hl, _ = world["lagrange"](n)
    assert lib.srs_lagrange_check(hl, world["h"], n, seed=SEED).ok  # warm
    before = lib.memory_stats()
    lib.fault_inject("launch:%d" % FAR)
    assert lib.srs_lagrange_check(hl, world["h"], n, seed=SEED).ok
    st = lib.fault_stats()
    lib.fault_inject(None)
    print("funnels of one warm check of %d rows:" % n, {k: st[k] for k in WARM})
    assert {k: st[k] for k in WARM} == WARM, st
    assert lib.memory_stats() == before


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, world, kind):
    """every site of the funnel `kind` that one warm check of 4096 rows passes, failed once.  These are host-side funnels; nothing faults on the device.  The
    call returns an error, no MSM ticket is outstanding, the live allocations and bytes are those of before, and the very next check is right."""
    from barretenberg_amd import BbGpuError
    n = 4096
    hl, _ = world["lagrange"](n)
    want = whole(lib.srs_lagrange_check(hl, world["h"], n, seed=SEED))  # warm
    assert want["ok"]
    before = lib.fault_stats()
    for k in range(WARM[KEYS[kind]] + 1):  # k == sites: the armed failure no longer fires
        lib.fault_inject("%s:%d" % (kind, k))
        if k < WARM[KEYS[kind]]:
            with pytest.raises(BbGpuError):
                lib.srs_lagrange_check(hl, world["h"], n, seed=SEED)
            st = lib.fault_stats()
            assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        else:
            assert whole(lib.srs_lagrange_check(hl, world["h"], n, seed=SEED)) == want
            st = lib.fault_stats()
            assert st["fired"] == 0 and st["armed"] == 1, (kind, k, st)
        lib.fault_inject(None)
        st = lib.fault_stats()
        assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        assert whole(lib.srs_lagrange_check(hl, world["h"], n, seed=SEED)) == want, (kind, k)
