"""bbgpu_g1_ntt and bbgpu_g1_recover on the GPU (-m gpu): the kernels of csrc/g1_recover.hip (k_g1_stage_cols, k_g1_load, k_g1_scale, k_g1_scalars,
k_g1_verdict, k_g1_finish) and the drivers in capi.hip against the host twins bit for bit, report included.  The twins themselves are held to the scalar
transform and the scalar decoder by tests/test_g1_recover_host.py.  Shapes:
  k_g1_stage_cols takes consecutive (column, group) pairs at one position while batch x groups >= 64 and consecutive positions below: (8, 3) and (8, 40)
  sit on both sides at every stage; at batch 1, 64 -> 128 crosses the switch in the first stage; (256, 3) has a batch that is no power of two, so that
  waves straddle positions and columns; (2, 1) is one butterfly.  The drivers take it up to n = 64 and k_lagrange_stage from 128 on
  (profiles/g1_recover.txt), so the shapes from 128 on run once as dispatched and once with bbgpu_g1_set_stage_mapping(2), the small ones also with 1;
  the ladder passes take position-major lane orders too: batch 70 at n = 8 is more than a wave per position.
Then infinity among the present points, a column of equal points, an altered point with and without redundancy, a round trip through the producer and the
checker over a 2-D layout, the bench's stage mapping, and the error contract under injected failures of the four host-side funnels (no failure is provoked
on the device)."""
import numpy as np
import pytest

from tests.g1_recover_cases import (INF, call_points, column_scalars, extended_world, missing_rows, output_buffer, points_of, present_rows)

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
# the funnels one warm bbgpu_g1_recover at (n, d, missing, batch) = (8, 4, 4, 3) passes (include/bbgpu.h): allocations -- the lists, z with z', the tables and
# the roots, the points, the findings, the two scratches; uploads -- the lists, the findings' start, the points; read-backs -- the findings, the points;
# launch checks -- k_recover_roots with k_recover_vanish, the batch inversion's two scans and its product, k_g1_scalars, k_g1_load, four transforms, three
# k_g1_scale passes, k_g1_verdict, k_g1_finish
WARM = dict(alloc_calls=5, h2d_calls=3, d2h_calls=2, launch_checks=15)
WARM_NTT = dict(alloc_calls=2, h2d_calls=1, d2h_calls=1, launch_checks=3)  # the points and the scratch; load, stages, finish


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.g1_set_stage_mapping(0)
    g.shutdown()


@pytest.mark.parametrize("kind", ["fft", "ifft"])
@pytest.mark.parametrize("n,batch", [(2, 1), (8, 3), (8, 40), (64, 2), (128, 1), (256, 3)])
def test_transform_equals_the_twin(lib, oracle, n, batch, kind):
    points = points_of(oracle, [v for col in column_scalars(n, n, batch) for v in col])
    kept = points.copy()
    got = lib.g1_ntt(points, n, kind, batch=batch)
    assert np.array_equal(points, kept) and np.array_equal(got, lib.host_g1_ntt(points, n, kind, batch=batch))


def test_transform_in_place_and_with_infinity(lib, oracle):
    n, batch = 8, 3
    cols = [list(v) for v in column_scalars(n, n, batch)]
    cols[1] = [0x51] * n  # equal points: the transform is (n P, inf, ..)
    cols[2][3] = 0        # infinity among the inputs
    points = points_of(oracle, [v for col in cols for v in col])
    want = lib.host_g1_ntt(points, n, "fft", batch=batch)
    assert sum(np.array_equal(p, INF) for p in want[1]) == n - 1
    buf = points.copy().reshape(batch, n, 8)
    assert lib.g1_ntt(buf, n, "fft", batch=batch, out=buf) is buf and np.array_equal(buf, want)


def both(lib, rows, points, n, d, batch):
    into = output_buffer(batch, n)
    got, got_rep = lib.g1_recover(rows, points, n, d, batch=batch, out=into)
    want, want_rep = lib.host_g1_recover(rows, points, n, d, batch=batch)
    assert got is into and np.array_equal(got, want) and got_rep == want_rep, (got_rep, want_rep)
    return got, got_rep


def case(oracle, n, d, mu, batch, alter=None, edit=None):
    rows = present_rows(n, missing_rows(n, mu))  # a shuffled order
    cols = [list(v) for v in column_scalars(n, d, batch)]
    if edit:
        edit(cols)
    if alter is not None:
        cols[alter[0]][int(rows[alter[1]])] += 1  # P_i + G
    return rows, cols, call_points(oracle, cols, rows)


@pytest.mark.parametrize("n,d,mu,batch", [(2, 1, 1, 1), (8, 4, 4, 70), (8, 4, 1, 3), (128, 64, 64, 2), (256, 100, 37, 3)])
def test_recover_equals_the_twin(lib, oracle, n, d, mu, batch):
    rows, cols, points = case(oracle, n, d, mu, batch)
    got, rep = both(lib, rows, points, n, d, batch)
    assert rep == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, missing=mu)
    for b, col in enumerate(cols):  # the twin's answer is the codeword the rows came from
        assert np.array_equal(got[b], points_of(oracle, col)), b


def test_infinity_among_the_present_points_and_a_column_of_equal_points(lib, oracle):
    n, d, mu, batch = 8, 4, 3, 4

    def edit(cols):
        cols[1][:] = [0xC0FFEE] * n  # every butterfly meets a doubling or a cancellation
        cols[2][:] = [0] * n         # a column at infinity
        cols[3][:] = [v - cols[3][int(rows_first)] for v in cols[3]]  # f - f(x): infinity at a listed row, degree unchanged
    rows_first = present_rows(n, missing_rows(n, mu))[0]
    rows, cols, points = case(oracle, n, d, mu, batch, edit=edit)
    assert np.array_equal(points[3 * len(rows)], INF)
    got, rep = both(lib, rows, points, n, d, batch)
    assert rep["consistent"] == 1
    for b, col in enumerate(cols):
        assert np.array_equal(got[b], points_of(oracle, col)), b


def test_one_altered_point_among_redundant_rows(lib, oracle):
    n, d, mu, batch = 256, 100, 37, 3
    rows, cols, points = case(oracle, n, d, mu, batch, alter=(2, 11))
    got, rep = both(lib, rows, points, n, d, batch)
    assert rep["consistent"] == 0 and rep["first_bad_column"] == 2 and d <= rep["first_bad_coeff"] < n - mu and rep["missing"] == mu
    for b in range(2):  # the other columns are not touched by it
        assert np.array_equal(got[b], points_of(oracle, cols[b])), b


def test_an_altered_point_without_redundancy_is_not_seen(lib, oracle):
    rows, cols, points = case(oracle, 8, 4, 4, 3, alter=(1, 2))
    _, rep = both(lib, rows, points, 8, 4, 3)
    assert rep == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, missing=4)


@pytest.mark.parametrize("mapping,n,batch", [(2, 128, 1), (2, 256, 3), (1, 8, 3), (1, 8, 40), (1, 64, 2)])
def test_either_stage_kernel_at_the_shapes_the_dispatch_gives_the_other(lib, oracle, mapping, n, batch):
    """bbgpu_g1_set_stage_mapping: 2 is k_g1_stage_cols for every shape -- from n = 128 on the dispatch takes k_lagrange_stage, and 64 -> 128 at batch 1 is
    where k_g1_stage_cols switches lane orders --, 1 is k_lagrange_stage with the column in blockIdx.y, the leg tools/g1_recover_bench.py compares with"""
    points = points_of(oracle, [v for col in column_scalars(n, n, batch) for v in col])
    want = {kind: lib.host_g1_ntt(points, n, kind, batch=batch) for kind in ("fft", "ifft")}
    lib.g1_set_stage_mapping(mapping)
    try:
        got = {kind: lib.g1_ntt(points, n, kind, batch=batch) for kind in ("fft", "ifft")}
    finally:
        lib.g1_set_stage_mapping(0)
    assert all(np.array_equal(got[kind], want[kind]) for kind in want)


@pytest.mark.parametrize("mapping", [1, 2])
def test_recover_by_either_stage_kernel(lib, oracle, mapping):
    rows, cols, points = case(oracle, 8, 4, 4, 70)
    lib.g1_set_stage_mapping(mapping)
    try:
        got, rep = lib.g1_recover(rows, points, 8, 4, batch=70)
    finally:
        lib.g1_set_stage_mapping(0)
    want, want_rep = lib.g1_recover(rows, points, 8, 4, batch=70)
    assert np.array_equal(got, want) and rep == want_rep and rep["consistent"] == 1


def test_round_trip_through_the_producer_and_the_checker(lib, oracle, tmp_path):
    """k = 4 polynomials at (256, 4) extended column-wise to 8 rows; rows {1, 2, 5, 6} are dropped.  bbgpu_g1_recover over the 65 columns -- the
    commitments' and one per cell -- returns all 8 x 65 points bit for bit, and bbgpu_kzg_check_open_cosets accepts the recovered commitments and proofs
    with the original values -- and rejects them after one recovered proof is replaced by its neighbour"""
    from tests.kzg_check_cells_cases import SEED, cosets_args
    W, columns = extended_world(lib, oracle, tmp_path)
    rows = np.array([7, 0, 4, 3], dtype=np.uint32)
    got, rep = lib.g1_recover(rows, np.ascontiguousarray(columns[:, rows]), 8, 4, batch=65)
    assert rep == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, missing=4) and np.array_equal(got, columns)
    commitments = np.ascontiguousarray(got[0])
    proofs = np.ascontiguousarray(got[1:].transpose(1, 0, 2))
    assert lib.kzg_check_open_cosets(*cosets_args(W, proofs=proofs, commitments=commitments), seed=SEED)["ok"] == 1
    proofs[5, 9] = proofs[5, 10]  # a recovered row's proof
    assert lib.kzg_check_open_cosets(*cosets_args(W, proofs=proofs, commitments=commitments), seed=SEED)["ok"] == 0


def warm_case(oracle):
    n, d, mu, batch = 8, 4, 4, 3
    rows, cols, points = case(oracle, n, d, mu, batch)
    return n, d, batch, rows, points, points_of(oracle, [v for col in cols for v in col]).reshape(batch, n, 8)


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_funnel_counts_of_a_warm_call(lib, oracle):
    n, d, batch, rows, points, want = warm_case(oracle)
    run = lambda: lib.g1_recover(rows, points, n, d, batch=batch)  # noqa: E731
    run()
    (got, rep), st = counted(lib, run, WARM)
    print("funnels of one warm g1_recover at (8, 4, 4, 3):", st)
    assert np.array_equal(got, want) and rep["consistent"] == 1 and st == WARM
    ntt = lambda: lib.g1_ntt(want, n, "ifft", batch=batch)  # noqa: E731
    ntt()
    _, st = counted(lib, ntt, WARM_NTT)
    print("funnels of one warm g1_ntt at (8, 3):", st)
    assert st == WARM_NTT


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, oracle, kind):
    """every site of the funnel `kind` that one warm call at (8, 4, 4, 3) passes, failed once.  These are host-side funnels (the library's failure injection
    of API results); nothing faults on the device.  Each failure returns an error, leaves no allocation live, the outputs as they were, and the next call
    is bit-exact."""
    import torch
    from barretenberg_amd import BbGpuError
    n, d, batch, rows, points, want = warm_case(oracle)

    def run(into=None):
        got, rep = lib.g1_recover(rows, points, n, d, batch=batch, out=into)
        torch.cuda.synchronize()
        return np.array_equal(got, want) and rep["consistent"] == 1
    assert run()  # warm
    _, sites = counted(lib, run, WARM)
    before = lib.fault_stats()
    for k in range(sites[KEYS[kind]] + 1):  # k == sites: the armed failure no longer fires
        lib.fault_inject("%s:%d" % (kind, k))
        if k < sites[KEYS[kind]]:
            into = output_buffer(batch, n)
            kept = into.copy()
            with pytest.raises(BbGpuError, match=" -1:"):
                run(into)
            st = lib.fault_stats()
            assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
            assert np.array_equal(into, kept) or (kind == "d2h" and k == sites[KEYS[kind]] - 1), (kind, k)  # the last read-back may have begun
        else:
            assert run(), (kind, k)
            st = lib.fault_stats()
            assert st["fired"] == 0 and st["armed"] == 1, (kind, k, st)
        lib.fault_inject(None)
        torch.cuda.synchronize()
        st = lib.fault_stats()
        assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        assert run(), (kind, k)


def test_kernel_times_are_reported(lib, oracle):
    n, d, batch, rows, points, _ = warm_case(oracle)
    lib.set_timing(1)
    try:
        lib.g1_recover(rows, points, n, d, batch=batch)
        times = lib.last_timing()
    finally:
        lib.set_timing(0)
    # the vanishing values; load and IFFT; shift, FFT, divide, IFFT, unshift and verdict; the last FFT and the finish; the finish alone, a part of the fourth
    assert len(times) == 5 and all(0 < v < 1000 for v in times) and times[4] < times[3], times
