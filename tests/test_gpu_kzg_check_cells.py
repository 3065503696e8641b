"""bbgpu_kzg_check_cells / bbgpu_kzg_check_open_cosets on the GPU (-m gpu): the kernels of csrc/kzg_check_cells.hip (k_kzg_cells,
k_kzg_cell_coefficients in both instantiations, k_kzg_cells_fold, k_kzg_cells_fold_finish) and the driver in capi.hip against the host twins
(csrc/host_kzg_check_cells.hpp), report against report, field for field, a and b included, under a fixed seed -- the twins themselves are held to an
independent reference by tests/test_kzg_check_cells_host.py.  l lanes take a cell, so the counts are chosen in cells around the edges of a wave (64 / l
cells) and of a workgroup (256 / l cells) for every l.  Past the grids: 33 x 2^14 and 64 x 2^14 cells of one point (k_kzg_cells' 2^19 threads), 5120 cells
of 64 points in the open-cosets form (the coefficient kernel's 1024 workgroups of 4 cells)."""
import numpy as np
import pytest

from oracle.pyoracle import aligned_copy
from tests.kzg_check_cells_cases import (INF, SEED, args_of, cells_of, cosets_args, honest, make_world, off_curve, padded, plus_one, power_of_secret, scalars,
                                         secret_x)
from tests.srs_check_cases import g2_of

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
COSETS = [1, 2, 4, 8, 16, 32, 64]
# the funnels one warm call of 256 cells at l = 4 passes (include/bbgpu.h).  Uploads: the proofs, the values, then the labels and the cell indices
# (labelled form), then the head (the roots, the findings' start value, the shared rows, P_0 .. P_3).  One read-back: the findings.  Launch checks:
# k_kzg_cells, k_kzg_cell_coefficients, k_kzg_cells_fold, and one per MSM ticket.  No allocation: the staging buffer and the MSM workspaces are kept.
WARM = {"labelled": dict(alloc_calls=0, h2d_calls=5, d2h_calls=1, launch_checks=5), "open_cosets": dict(alloc_calls=0, h2d_calls=3, d2h_calls=1, launch_checks=5)}
# with a finding: no fold and no ticket -- three launch checks fewer
WARM_FINDING = dict(alloc_calls=0, h2d_calls=5, d2h_calls=1, launch_checks=2)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def worlds(lib, oracle, tmp_path_factory):
    """host-made worlds per (n, l, batch), made on first use, never written to"""
    made = {}

    def world(n, l, batch=3):
        if (n, l, batch) not in made:
            made[(n, l, batch)] = make_world(lib, oracle, tmp_path_factory.mktemp("cells_%d_%d_%d" % (n, l, batch)), n, l, batch)
        return made[(n, l, batch)]
    return world


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def device_world(lib, oracle, tmp_path, n, l, batch):
    """batch polynomials of n coefficients committed to, transformed and opened on every coset BY THE DEVICE (bbgpu_msm_g1_device, bbgpu_ntt_device_batch,
    bbgpu_kzg_open_cosets_device): commitments (batch, 8), values (batch, n, 4), proofs (batch, n / l, 8)"""
    import torch
    h, table = lib.srs_generate(secret_x(oracle), n, want_host_table=True)
    try:
        c = aligned_copy(oracle.random_scalars(0xD0C + n + l, batch * n))
        d_c = dev(c)
        setup = lib.kzg_open_cosets_setup(h, n, l)
        try:
            proofs = lib.kzg_open_cosets_device(setup, d_c.data_ptr(), n, l, batch=batch)
        finally:
            lib.kzg_open_cosets_release(setup)
        d_y = d_c.clone()
        torch.cuda.synchronize()
        commitments = np.stack([lib.msm_device(h, d_c.data_ptr() + b * n * 32, n)[:8] for b in range(batch)])
        lib.ntt_device_batch(d_y.data_ptr(), n, batch, "fft")
        torch.cuda.synchronize()
        return dict(n=n, l=l, m=n // l, batch=batch, head=aligned_copy(table[0:2 * l:2]), commitments=commitments, proofs=proofs,
                    g2_xl=g2_of(lib, oracle, tmp_path, power_of_secret(oracle, l), "xl.dat"), values=d_y.cpu().numpy().view(np.uint64).reshape(batch, n, 4))
    finally:
        lib.srs_release(h)


def both(lib, W, which, cell, values, proofs, commitments=None, **kw):
    """(device report, twin report) of one call in the labelled form"""
    a = args_of(W, which, cell, values, proofs, commitments=commitments)
    return lib.kzg_check_cells(*a, seed=SEED, **kw), lib.host_kzg_check_cells(*a, seed=SEED, **kw)


def both_cosets(lib, W, stride=None, **kw):
    opts = {k: kw.pop(k) for k in ("locate",) if k in kw}
    a = cosets_args(W, **kw)
    return lib.kzg_check_open_cosets(*a, stride=stride, seed=SEED, **opts), lib.host_kzg_check_open_cosets(*a, stride=stride, seed=SEED, **opts)


def false_value(oracle, values, l, t, j):
    v = values.copy()
    v[t * l + j] = plus_one(oracle, v[t * l + j])
    return v


@pytest.mark.parametrize("l", COSETS)
def test_lane_group_edges(lib, oracle, worlds, l):
    """cells around the edges of a wave and of a workgroup, honest, and with one false value in the middle cell under LOCATE: the whole report"""
    W = worlds(16 * l, l)
    for count in sorted({c for c in (1, 64 // l - 1, 64 // l, 64 // l + 1, 256 // l - 1, 256 // l, 256 // l + 1) if c >= 1}):
        which, cell, values, proofs = cells_of(W, count, start=count)
        got, want = both(lib, W, which, cell, values, proofs)
        assert got == want and scalars(got) == honest(count), (count, got, want)
        got, want = both(lib, W, which, cell, false_value(oracle, values, l, count // 2, l // 2), proofs, locate=True)
        assert got == want and got["ok"] == 0 and got["first_failing"] == count // 2, (count, got, want)
    assert lib.fault_stats()["slots_pending"] == 0


@pytest.mark.parametrize("l", [4, 64])
def test_false_values_at_chosen_positions(lib, oracle, worlds, l):
    """the first cell, the last of the first wave, the first of the second wave, the first of the second workgroup, the last; the first and the last value"""
    W = worlds(16 * l, l)
    count = 256 // l + 64 // l + 3
    which, cell, values, proofs = cells_of(W, count)
    for t in sorted({0, 64 // l - 1, 64 // l, 256 // l, count - 1}):
        for j in sorted({0, l - 1}):
            got, want = both(lib, W, which, cell, false_value(oracle, values, l, t, j), proofs, locate=True)
            assert got == want and got["ok"] == 0 and got["first_failing"] == t, (t, j, got)
    assert both(lib, W, which, cell, false_value(oracle, values, l, 1, 0), proofs)[0]["first_failing"] == -1  # without the flag nothing is located


@pytest.mark.parametrize("n,l,batch,pad", [(2, 1, 1, 0), (128, 64, 1, 0), (256, 4, 3, 5), (4096, 64, 5, 0)])
def test_open_cosets_form(lib, oracle, tmp_path, n, l, batch, pad):
    """what the device wrote (bbgpu_msm_g1_device, bbgpu_ntt_device_batch, bbgpu_kzg_open_cosets_device) is accepted, the report is the twin's; then a
    value of the last polynomial is falsified and located"""
    V = device_world(lib, oracle, tmp_path, n, l, batch)
    m = n // l
    buf, stride = padded(oracle, V, pad)
    got, want = both_cosets(lib, V, values=buf, stride=stride)
    assert got["ok"] == 1 and got == want and scalars(got) == honest(batch * m), (got, want)
    k, j = m - 2, l - 1  # cell k of the last polynomial, its last value
    buf[(batch - 1) * stride + k + m * j] = plus_one(oracle, buf[(batch - 1) * stride + k + m * j])
    got, want = both_cosets(lib, V, values=buf, stride=stride, locate=True)
    assert got == want and got["ok"] == 0 and got["first_failing"] == (batch - 1) * m + k, (got, want)


def test_cosets_of_one_point_are_the_open_all_check(lib, oracle, worlds):
    """l = 1: the report of bbgpu_kzg_check_open_all on the same data, honest and with a false value located"""
    W = worlds(64, 1)
    assert np.array_equal(W["g2_xl"], W["g2_x"])
    values = aligned_copy(W["values"].reshape(-1, 4))
    got = lib.kzg_check_open_cosets(*cosets_args(W, values=values), seed=SEED)
    assert got == lib.kzg_check_open_all(W["commitments"], values, W["proofs"], 64, W["g2_x"], seed=SEED) and scalars(got) == honest(192)
    values[100] = plus_one(oracle, values[100])
    got = lib.kzg_check_open_cosets(*cosets_args(W, values=values), seed=SEED, locate=True)
    assert got == lib.kzg_check_open_all(W["commitments"], values, W["proofs"], 64, W["g2_x"], seed=SEED, locate=True) and got["first_failing"] == 100


def test_second_trip_of_the_stride_loop(lib, oracle, worlds):
    """4100 cells at l = 64 (262,400 values, within the 2^20 bound): the coefficient kernel's 1024 workgroups of 4 cells take a second trip, the fold
    takes two ranges and the finish kernel.  Against the twin only."""
    W = worlds(1024, 64)
    count = 4100
    which, cell, values, proofs = cells_of(W, count)
    got, want = both(lib, W, which, cell, values, proofs)
    assert got == want and scalars(got) == honest(count)
    got, want = both(lib, W, which, cell, false_value(oracle, values, 64, 4098, 63), proofs, locate=True)
    assert got == want and got["first_failing"] == 4098


@pytest.fixture(scope="module")
def one_point_world(lib, oracle, tmp_path_factory):
    """(n, l, batch) = (2^14, 1, 64) by the device producers: 2^20 cells of one point.  Made once, never written to."""
    return device_world(lib, oracle, tmp_path_factory.mktemp("cells_of_one_point"), 1 << 14, 1, 64)


@pytest.mark.parametrize("batch", [33, 64])
def test_cosets_of_one_point_past_the_cell_grid(lib, oracle, one_point_world, batch):
    """l = 1 at 33 x 2^14 and 64 x 2^14 cells: k_kzg_cells' 2^19 threads take a partial and a full second trip, the 1024 workgroups of 256 cells of the
    coefficient kernel more than two, the fold all its ranges.  The report is bbgpu_kzg_check_open_all's on the same data ([x^1] G2 is x G2), honest and
    with a false value at cell 2^19 + 100 located."""
    V, n, t = one_point_world, 1 << 14, (1 << 19) + 100
    cs, proofs, values = V["commitments"][:batch], V["proofs"][:batch], aligned_copy(V["values"][:batch].reshape(-1, 4))
    got = lib.kzg_check_open_cosets(cs, values, proofs, n, 1, V["head"], V["g2_xl"], seed=SEED)
    assert got == lib.kzg_check_open_all(cs, values, proofs, n, V["g2_xl"], seed=SEED) and scalars(got) == honest(batch * n)
    values[t] = plus_one(oracle, values[t])
    got = lib.kzg_check_open_cosets(cs, values, proofs, n, 1, V["head"], V["g2_xl"], seed=SEED, locate=True)
    assert got == lib.kzg_check_open_all(cs, values, proofs, n, V["g2_xl"], seed=SEED, locate=True)
    assert got["ok"] == 0 and got["first_failing"] == t and got["count"] == batch * n, got


def test_second_trip_of_the_transposed_load(lib, oracle, tmp_path):
    """(n, l, batch) = (2^16, 64, 5) by the device producers: 5120 cells, 327,680 values, so the 1024 workgroups of 4 cells of the open-cosets form of the
    coefficient kernel take a second trip through their transposed load.  Device against twin, field for field, with padding between the polynomials;
    then a false value in cell 4097 (its last point) and in the last cell, each located exactly."""
    n, l, batch = 1 << 16, 64, 5
    V = device_world(lib, oracle, tmp_path, n, l, batch)
    m = n // l
    buf, stride = padded(oracle, V, 5)
    got, want = both_cosets(lib, V, values=buf, stride=stride)
    assert got["ok"] == 1 and got == want and scalars(got) == honest(batch * m), (got, want)
    for t, j in ((4097, l - 1), (batch * m - 1, 0)):
        b, k = t // m, t % m
        false = buf.copy()
        false[b * stride + k + m * j] = plus_one(oracle, false[b * stride + k + m * j])
        got, want = both_cosets(lib, V, values=false, stride=stride, locate=True)
        assert got == want and got["ok"] == 0 and got["first_failing"] == t, (t, got, want)


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_points_off_the_curve_are_findings(lib, oracle, worlds):
    """off-curve points on both sides of a wave edge of 300 cells at l = 1 and of 40 at l = 4: counts and the first finding are exact, and neither the fold
    nor a ticket is issued (two launch checks: k_kzg_cells and k_kzg_cell_coefficients)"""
    for l, count, edge in ((1, 300, 64), (4, 40, 16)):
        W = worlds(16 * l, l)
        which, cell, values, proofs = cells_of(W, count)
        for spots in ((edge - 1,), (edge,), (edge - 1, edge), (edge, count - 1)):
            p2 = proofs.copy()
            for t in spots:
                p2[t] = off_curve(oracle, proofs[t])
            lib.kzg_check_cells(*args_of(W, which, cell, values, p2), seed=SEED)  # warm
            (got, want), st = counted(lib, lambda: both(lib, W, which, cell, values, p2, locate=True), WARM_FINDING)
            assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=len(spots), first_bad=spots[0], first_bad_is_proof=1), (l, got)
            assert st == WARM_FINDING and lib.fault_stats()["slots_pending"] == 0, st
        sh = W["commitments"].copy()
        sh[2] = off_curve(oracle, sh[2])
        got, want = both(lib, W, which, cell, values, proofs, commitments=sh)  # a commitment alone
        assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=1, first_bad=2, first_bad_is_proof=0)
        p2 = proofs.copy()
        p2[0] = off_curve(oracle, proofs[0])
        got, want = both(lib, W, which, cell, values, p2, commitments=sh)  # both: a shared commitment comes before any cell
        assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=2, first_bad=2, first_bad_is_proof=0)
        got, want = both(lib, W, which, cell, values, proofs)  # the next call is the honest one
        assert got == want and got["ok"] == 1


def test_infinities_and_duplicates(lib, oracle, tmp_path):
    """degree < l: every proof at infinity, A and B at infinity; the zero polynomial: a commitment at infinity; the same cell many times"""
    n, l, m = 64, 4, 16
    rnd = oracle.random_scalars(0x5BEC, 3 * n).reshape(3, n, 4).copy()
    rnd[0, l:] = 0
    rnd[1] = 0
    W = make_world(lib, oracle, tmp_path, n, l, 3, coeffs=rnd)
    inf = [int(v) for v in INF]
    assert np.array_equal(W["proofs"][:2], np.tile(INF, (2, m, 1))) and np.array_equal(W["commitments"][1], INF)
    got, want = both_cosets(lib, W)
    assert got == want and scalars(got) == honest(3 * m)
    V = dict(W, commitments=W["commitments"][:2], values=W["values"][:2], proofs=W["proofs"][:2], batch=2)
    got, want = both_cosets(lib, V)
    assert got == want and scalars(got) == honest(2 * m) and got["a"] == inf and got["b"] == inf
    which, cell, values, proofs = cells_of(W, 300)  # 48 distinct cells: colliding rows in both MSMs
    got, want = both(lib, W, which, cell, values, proofs)
    assert got == want and scalars(got) == honest(300)


def test_seed_rules_and_determinism(lib, worlds):
    W = worlds(64, 4)
    runs = [lib.kzg_check_open_cosets(*cosets_args(W), seed=SEED) for _ in range(2)]
    assert runs[0] == runs[1]
    drawn = [lib.kzg_check_open_cosets(*cosets_args(W)) for _ in range(2)]
    assert all(r["ok"] == 1 for r in drawn) and drawn[0]["seed"] != drawn[1]["seed"] and drawn[0]["a"] != drawn[1]["a"]
    assert lib.host_kzg_check_open_cosets(*cosets_args(W), seed=np.array(drawn[0]["seed"], dtype=np.uint64)) == drawn[0]


def calls(lib, oracle, worlds, falsify=None):
    """256 cells at l = 4 in both forms; falsify: the cell whose first value is changed"""
    W = worlds(1024, 4, 1)
    which, cell, values, proofs = cells_of(W, 256)
    transforms = aligned_copy(W["values"].reshape(-1, 4))
    if falsify is not None:
        values = false_value(oracle, values, 4, falsify, 0)
        transforms[falsify] = plus_one(oracle, transforms[falsify])  # cell k = falsify, j = 0
    return {"labelled": lambda **kw: both(lib, W, which, cell, values, proofs, **kw), "open_cosets": lambda **kw: both_cosets(lib, W, values=transforms, **kw)}


def test_funnel_counts_of_warm_calls(lib, oracle, worlds):
    """256 cells at l = 4 in each form: the counts of include/bbgpu.h; the staging is counted in bbgpu_memory_stats"""
    for form, run in calls(lib, oracle, worlds).items():
        run()  # warm
        (got, want), st = counted(lib, run, WARM[form])  # the twin makes no HIP call: the counts are the device call's
        print("funnels of one warm call of 256 cells at l = 4,", form, st)
        assert got == want and got["ok"] == 1 and st == WARM[form], (form, st)
    assert lib.memory_stats()["staging_bytes"] >= 256 * (64 + 4 * 64)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["labelled", "open_cosets"])
def test_injected_failures_leave_nothing_behind(lib, oracle, worlds, form, kind):
    """every site of the funnel `kind` that one warm call with LOCATE over a false cell passes (fold and MSM rounds included), failed once.  These are
    the library's injected error returns; nothing faults on the device.  Each failure is an error return with no MSM slot pending, the live allocations
    of before and a staging that does not grow, and the very next call gives the honest report."""
    from barretenberg_amd import BbGpuError
    both_reports = calls(lib, oracle, worlds, falsify=200)[form]
    run = lambda: both_reports(locate=True)[0]  # noqa: E731
    want = both_reports(locate=True)[1]
    assert run() == want and want["first_failing"] == 200  # warm
    lib.fault_inject("%s:%d" % (kind, FAR))
    assert run() == want
    st = lib.fault_stats()
    sites, live, staging = st[KEYS[kind]], st["live_allocations"], lib.memory_stats()["staging_bytes"]
    assert sites >= WARM[form][KEYS[kind]], st
    for k in range(sites):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError, match=" -1:"):
            run()
        st = lib.fault_stats()
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["slots_pending"] == 0 and st["live_allocations"] == live and lib.memory_stats()["staging_bytes"] == staging, (kind, k, st)
        assert run() == want, (kind, k)
    lib.fault_inject(None)


def test_the_stage_timing_of_the_last_call(lib, worlds):
    """bbgpu_kzg_check_last_timing (diagnostic) also reports these entries: non-negative wall times that add up to the total"""
    W = worlds(64, 4)
    assert lib.kzg_check_open_cosets(*cosets_args(W), seed=SEED)["ok"] == 1
    ms = lib.kzg_check_last_timing()
    assert all(v >= 0 for v in ms.values()) and ms["total_ms"] > 0 and ms["claims_ms"] > 0 and ms["msm_ms"] > 0 and ms["host_tail_ms"] > 0
    assert abs(ms["total_ms"] - sum(v for k, v in ms.items() if k != "total_ms")) < 1e-6
