"""bbgpu_g1_recover_each on the GPU (-m gpu): k_g1_roots and k_g1_vanish_cols of csrc/g1_recover.hip, the per-column forms of k_g1_scalars, k_g1_load,
k_g1_scale and k_g1_verdict, and the driver in capi.hip against the host twin bit for bit, report and first_bad included.  The twin itself is held to the
scalar decoder by tests/test_g1_recover_each_host.py.  Shapes (n, d, missing per column):
  (2, 1)      1, 0, 1                one butterfly; a column that misses nothing between two that do
  (8, 4)      b mod 5, 70 columns    more than a wave per position in the ladder passes; 32 columns per workgroup of k_g1_vanish_cols, the last
                                     workgroup short, columns with nothing missing among them
  (64, 17)    0, 1, 30, 47, 47       a full wave per column; two different sets of 47
  (128, 64)   64, 1, 33              two columns per vanish workgroup, the last one short; the dispatch takes k_lagrange_stage
  (256, 100)  37, 0, 156             one column per workgroup
  (512, 100)  300, 5                 a list longer than one LDS tile beside a short one
Then the same set for all columns against bbgpu_g1_recover, special points, findings, a round trip through the producer and the checker over a 2-D layout
with a different set of rows per column, the stage kernels, and the error contract under injected failures of the four host-side funnels (no failure is
provoked on the device)."""
import numpy as np
import pytest

from tests.g1_recover_cases import INF, call_points, extended_world, missing_rows, present_rows
from tests.g1_recover_each_cases import NONE, clean_report, column_scalars, each_case, output_buffer, points_of

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
# the funnels one warm bbgpu_g1_recover_each at (n, d, batch) = (8, 4, 3), missing 4, 3, 1, passes (include/bbgpu.h): allocations -- the lists, z with z',
# the tables and the roots, the points, the findings, the two scratches; uploads -- the lists, the findings' start, the points; read-backs -- the findings,
# the points; launch checks -- k_g1_roots with k_g1_vanish_cols, the batch inversion's two scans and its product, k_g1_scalars, k_g1_load, four transforms,
# three k_g1_scale passes, k_g1_verdict, k_g1_finish
WARM = dict(alloc_calls=5, h2d_calls=3, d2h_calls=2, launch_checks=15)
SHAPES = [(2, 1, (1, 0, 1)), (8, 4, tuple(b % 5 for b in range(70))), (64, 17, (0, 1, 30, 47, 47)), (128, 64, (64, 1, 33)), (256, 100, (37, 0, 156)),
          (512, 100, (300, 5))]


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.g1_set_stage_mapping(0)
    g.shutdown()


def both(lib, rows, points, n, d):
    batch = len(rows)
    into = output_buffer(batch, n)
    got, got_rep, got_bad = lib.g1_recover_each(rows, points, n, d, out=into)
    want, want_rep, want_bad = lib.host_g1_recover_each(rows, points, n, d)
    assert got is into and np.array_equal(got, want) and got_rep == want_rep and np.array_equal(got_bad, want_bad), (got_rep, want_rep, got_bad, want_bad)
    return got, got_rep, got_bad


@pytest.mark.parametrize("n,d,mus", SHAPES, ids=["2", "8x70", "64", "128", "256", "512"])
def test_recover_each_equals_the_twin(lib, oracle, n, d, mus):
    rows, cols, points = each_case(oracle, n, d, mus)
    got, rep, first_bad = both(lib, rows, points, n, d)
    assert rep == clean_report(mus) and all(int(v) == NONE for v in first_bad)
    for b, col in enumerate(cols):  # the twin's answer is the codeword the rows came from
        assert np.array_equal(got[b], points_of(oracle, col)), b


@pytest.mark.parametrize("n,d,mu,batch", [(8, 4, 4, 70), (256, 100, 37, 3)])
def test_the_same_set_for_all_columns_equals_g1_recover(lib, oracle, n, d, mu, batch):
    shared = present_rows(n, missing_rows(n, mu))
    cols = [list(v) for v in column_scalars(n, d, batch)]
    points = call_points(oracle, cols, shared)
    want, want_rep = lib.g1_recover(shared, points, n, d, batch=batch)
    got, rep, first_bad = lib.g1_recover_each([shared] * batch, points, n, d)  # one array, in the order of the lists
    assert np.array_equal(got, want) and all(int(v) == NONE for v in first_bad)
    assert rep == dict(consistent=want_rep["consistent"], first_bad_column=want_rep["first_bad_column"], first_bad_coeff=want_rep["first_bad_coeff"],
                       max_missing=want_rep["missing"]) == clean_report([mu])


def test_infinity_among_the_present_points_a_column_of_equal_points_and_a_column_at_infinity(lib, oracle):
    n, d, mus = 8, 4, (3, 2, 4, 1)

    def edit(cols, rows):
        cols[1][:] = [0xC0FFEE] * n  # every butterfly meets a doubling or a cancellation
        cols[2][:] = [0] * n         # a column at infinity
        cols[3][:] = [v - cols[3][int(rows[3][0])] for v in cols[3]]  # f - f(x): infinity at a listed row, degree unchanged
    rows, cols, points = each_case(oracle, n, d, mus, edit=edit)
    assert np.array_equal(points[3][0], INF)
    got, rep, first_bad = both(lib, rows, points, n, d)
    assert rep == clean_report(mus)
    for b, col in enumerate(cols):
        assert np.array_equal(got[b], points_of(oracle, col)), b


def test_findings_in_their_columns_only(lib, oracle):
    """(64, 17), missing 0, 1, 30, 47, 47: an altered point among redundant rows is found in its column only; where a column lists exactly d rows it is not
    seen; two bad columns are both in first_bad and the report names the first"""
    n, d, mus = 64, 17, (0, 1, 30, 47, 47)
    clean = column_scalars(n, d, len(mus))
    rows, cols, points = each_case(oracle, n, d, mus, alter=[(2, 11)])
    got, rep, first_bad = both(lib, rows, points, n, d)
    assert rep["consistent"] == 0 and rep["first_bad_column"] == 2 and d <= rep["first_bad_coeff"] < n - 30 and rep["max_missing"] == 47
    assert [int(v) != NONE for v in first_bad] == [False, False, True, False, False] and int(first_bad[2]) == rep["first_bad_coeff"]
    for b in (0, 1, 3, 4):  # the other columns are not touched by it
        assert np.array_equal(got[b], points_of(oracle, clean[b])), b
    rows, cols, points = each_case(oracle, n, d, mus, alter=[(3, 5)])  # count == d: no redundancy
    got, rep, first_bad = both(lib, rows, points, n, d)
    assert rep == clean_report(mus) and all(int(v) == NONE for v in first_bad)
    rows, cols, points = each_case(oracle, n, d, mus, alter=[(2, 11), (1, 40)])
    got, rep, first_bad = both(lib, rows, points, n, d)
    assert rep["consistent"] == 0 and rep["first_bad_column"] == 1 and rep["first_bad_coeff"] == int(first_bad[1])
    assert [int(v) != NONE for v in first_bad] == [False, True, True, False, False]


def test_round_trip_through_the_producer_and_the_checker(lib, oracle, tmp_path):
    """k = 4 polynomials at (256, 4) extended column-wise to 8 rows; every one of the 65 columns -- the commitments' and one per cell -- keeps its own seeded
    set of 4 to 6 rows.  bbgpu_g1_recover_each returns all 8 x 65 points bit for bit, and bbgpu_kzg_check_open_cosets accepts the recovered commitments and
    proofs with the original values -- and rejects them after one recovered proof is replaced by its neighbour"""
    from tests.kzg_check_cells_cases import SEED, cosets_args
    W, columns = extended_world(lib, oracle, tmp_path)
    rng = np.random.default_rng(0x2D65)
    rows = [rng.permutation(8)[:4 + c % 3].astype(np.uint32) for c in range(65)]
    assert len({tuple(sorted(int(k) for k in r)) for r in rows}) > 30
    points = [np.ascontiguousarray(columns[c, r]) for c, r in enumerate(rows)]
    got, rep, first_bad = lib.g1_recover_each(rows, points, 8, 4)
    assert rep == dict(consistent=1, first_bad_column=0, first_bad_coeff=0, max_missing=4) and all(int(v) == NONE for v in first_bad)
    assert np.array_equal(got, columns)
    commitments = np.ascontiguousarray(got[0])
    proofs = np.ascontiguousarray(got[1:].transpose(1, 0, 2))
    assert lib.kzg_check_open_cosets(*cosets_args(W, proofs=proofs, commitments=commitments), seed=SEED)["ok"] == 1
    proofs[5, 9] = proofs[5, 10]
    assert lib.kzg_check_open_cosets(*cosets_args(W, proofs=proofs, commitments=commitments), seed=SEED)["ok"] == 0


@pytest.mark.parametrize("mapping", [1, 2])
def test_recover_each_by_either_stage_kernel(lib, oracle, mapping):
    n, d, mus = SHAPES[1]
    rows, cols, points = each_case(oracle, n, d, mus)
    lib.g1_set_stage_mapping(mapping)
    try:
        got, rep, first_bad = lib.g1_recover_each(rows, points, n, d)
    finally:
        lib.g1_set_stage_mapping(0)
    want, want_rep, want_bad = lib.g1_recover_each(rows, points, n, d)
    assert np.array_equal(got, want) and rep == want_rep == clean_report(mus) and np.array_equal(first_bad, want_bad)


def warm_case(oracle):
    n, d, mus = 8, 4, (4, 3, 1)
    rows, cols, points = each_case(oracle, n, d, mus)
    return n, d, rows, points, points_of(oracle, [v for col in cols for v in col]).reshape(len(mus), n, 8)


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_funnel_counts_of_a_warm_call(lib, oracle):
    n, d, rows, points, want = warm_case(oracle)
    run = lambda: lib.g1_recover_each(rows, points, n, d)  # noqa: E731
    run()
    (got, rep, first_bad), st = counted(lib, run, WARM)
    print("funnels of one warm g1_recover_each at (8, 4, 3), missing 4, 3, 1:", st)
    assert np.array_equal(got, want) and rep["consistent"] == 1 and st == WARM


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, oracle, kind):
    """every site of the funnel `kind` that one warm call at (8, 4, 3) passes, failed once.  These are host-side funnels (the library's failure injection
    of API results); nothing faults on the device.  Each failure returns an error, leaves no allocation live, the outputs as they were, and the next call
    is bit-exact."""
    import torch
    from barretenberg_amd import BbGpuError
    n, d, rows, points, want = warm_case(oracle)
    batch = len(rows)

    def run(into=None):
        got, rep, first_bad = lib.g1_recover_each(rows, points, n, d, out=into)
        torch.cuda.synchronize()
        return np.array_equal(got, want) and rep["consistent"] == 1 and all(int(v) == NONE for v in first_bad)
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
    n, d, rows, points, _ = warm_case(oracle)
    lib.set_timing(1)
    try:
        lib.g1_recover_each(rows, points, n, d)
        times = lib.last_timing()
    finally:
        lib.set_timing(0)
    # roots and k_g1_vanish_cols; load and IFFT; shift through verdict; the last FFT and the finish; the finish alone, a part of the fourth
    assert len(times) == 5 and all(0 < v < 1000 for v in times) and times[4] < times[3], times
