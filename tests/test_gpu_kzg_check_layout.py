"""bbgpu_kzg_check_cells_layout / bbgpu_kzg_check_open_cosets_layout on the GPU (-m gpu): the kernels of the last section of csrc/kzg_check_cells.hip
(k_kzg_layout_commitments, k_kzg_layout_hist, k_kzg_layout_scan, k_kzg_layout_scatter, k_kzg_layout_pieces, k_kzg_layout_finish) and the `layout` path of
the driver in capi.hip against the host twins, report against report, field for field, a and b included, under a fixed seed -- the twins are held to an
independent reference by tests/test_kzg_check_layout_host.py.  Labels >= 64 are what a fold that kept the 64 slots would get wrong.  The sizes: lists of
0, 1, 1024 +- and 4097 cells (a wave takes a piece of at most 1024 cells), S around the edges of a wave of commitments (64) and of the scan's 256 threads
(S = 257: two counters on some threads; 4099; 2^16: 256 each)."""
import numpy as np
import pytest

from oracle.pyoracle import aligned_copy
from tests.kzg_check_cells_cases import INF, SEED, args_of, cosets_args, cosets_as_labelled, honest, make_world, off_curve, padded, plus_one, scalars
from tests.kzg_check_layout_cases import MAX_S, PIECE, cells_under, commitments_of, make_worlds, mixed, patterns, rows_world, uniform

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
COSETS = [1, 2, 4, 8, 16, 32, 64]
# the funnels one warm call of 256 cells at l = 4 passes (include/bbgpu.h).  Uploads: the proofs, the values, then the labels and the cell indices
# (labelled form), the commitments, the head.  One read-back: the findings of cells and commitments.  Launch checks: k_kzg_cells,
# k_kzg_cell_coefficients, the commitments with the grouping, k_kzg_cells_fold, the grouped fold, and one per MSM ticket.  No allocation.
WARM = {"labelled": dict(alloc_calls=0, h2d_calls=6, d2h_calls=1, launch_checks=7), "open_cosets": dict(alloc_calls=0, h2d_calls=4, d2h_calls=1, launch_checks=7)}
# with a finding: no fold and no ticket
WARM_FINDING = {"labelled": dict(alloc_calls=0, h2d_calls=6, d2h_calls=1, launch_checks=3), "open_cosets": dict(alloc_calls=0, h2d_calls=4, d2h_calls=1, launch_checks=3)}


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def worlds(lib, oracle, tmp_path_factory):
    return make_worlds(lib, oracle, tmp_path_factory)


def both(lib, W, S, cells, commitments=None, **kw):
    """(device report, twin report) of one layout call in the labelled form"""
    a = args_of(W, *cells, commitments=commitments_of(W, S) if commitments is None else commitments)
    return lib.kzg_check_cells_layout(*a, seed=SEED, **kw), lib.host_kzg_check_cells_layout(*a, seed=SEED, **kw)


def both_cosets(lib, V, stride=None, locate=False, **kw):
    a = cosets_args(V, **kw)
    return (lib.kzg_check_open_cosets_layout(*a, stride=stride, seed=SEED, locate=locate),
            lib.host_kzg_check_open_cosets_layout(*a, stride=stride, seed=SEED, locate=locate))


@pytest.mark.parametrize("l", COSETS)
def test_up_to_64_commitments_the_reports_are_the_old_entries(lib, oracle, worlds, l):
    """every l at the smallest n, S = 8 and 64, both forms: the layout entry, bbgpu_kzg_check_cells / _open_cosets and the twin agree field for field"""
    W = worlds(2 * l, l)
    for S in (8, 64):
        cells = cells_under(W, mixed(S, 70))
        a = args_of(W, *cells, commitments=commitments_of(W, S))
        got = lib.kzg_check_cells_layout(*a, seed=SEED)
        assert got == lib.kzg_check_cells(*a, seed=SEED) == lib.host_kzg_check_cells_layout(*a, seed=SEED) and scalars(got) == honest(70), (S, got)
        v2 = cells[2].copy()
        v2[33 * l] = plus_one(oracle, v2[33 * l])
        a = args_of(W, cells[0], cells[1], v2, cells[3], commitments=commitments_of(W, S))
        got = lib.kzg_check_cells_layout(*a, seed=SEED, locate=True)
        assert got == lib.kzg_check_cells(*a, seed=SEED, locate=True) and got["ok"] == 0 and got["first_failing"] == 33, (S, got)
    V = rows_world(W, 64)
    got, want = both_cosets(lib, V)
    assert got == want == lib.kzg_check_open_cosets(*cosets_args(V), seed=SEED) and scalars(got) == honest(64 * W["m"]), got


@pytest.mark.parametrize("n,l,S,count", [(16, 4, 65, 5000), (16, 4, 257, 5000), (16, 4, 4099, 5000), (128, 64, 257, 4500)])
def test_label_patterns(lib, oracle, worlds, n, l, S, count):
    """uniform labels, every cell on the last label, one list of 4097 cells among spread ones, labels below 64 under 4099 commitments: the twin's report"""
    W = worlds(n, l)
    for name, labels in patterns(S, count).items():
        got, want = both(lib, W, S, cells_under(W, labels))
        assert got == want and scalars(got) == honest(count), (name, got, want)
    assert lib.fault_stats()["slots_pending"] == 0


def test_lists_around_a_piece(lib, oracle, worlds):
    """one list of 1023, 1024 and 1025 cells under label 100 of 130, the other cells on label 129: a full piece, and a second piece of one cell"""
    W = worlds(16, 4)
    for length in (PIECE - 1, PIECE, PIECE + 1):
        labels = np.full(length + 37, 129)
        labels[np.arange(length) + np.arange(length) // 40] = 100
        assert (labels == 100).sum() == length
        got, want = both(lib, W, 130, cells_under(W, labels))
        assert got == want and scalars(got) == honest(length + 37), (length, got, want)


def test_the_most_commitments(lib, oracle, worlds):
    """S = 2^16 exactly over 2^16 + 3 cells at l = 4: every label but three owns one cell"""
    W = worlds(16, 4)
    count = MAX_S + 3
    got, want = both(lib, W, MAX_S, cells_under(W, uniform(MAX_S, count)))
    assert got == want and scalars(got) == honest(count), (got, want)


@pytest.mark.parametrize("n,l", [(16, 4), (128, 64)])
def test_false_claims_under_labels_above_64(lib, oracle, worlds, n, l):
    """a false value, a false proof, a false commitment: rejected, and located as the twin locates them"""
    W = worlds(n, l)
    S, count = 257, 1500
    labels = uniform(S, count)
    which, cell, values, proofs = cells_under(W, labels)
    t = int(np.flatnonzero(labels == 203)[1])
    assert t > 64
    v2 = values.copy()
    v2[t * l + l - 1] = plus_one(oracle, v2[t * l + l - 1])
    p2 = proofs.copy()
    p2[t] = proofs[t - 1]
    assert not np.array_equal(proofs[t], proofs[t - 1])
    cs = commitments_of(W, S)
    cs[203] = W["commitments"][(203 + 1) % 8]
    first = int(np.flatnonzero(labels == 203)[0])
    for cells, commitments, where in (((which, cell, v2, proofs), None, t), ((which, cell, values, p2), None, t), ((which, cell, values, proofs), cs, first)):
        got, want = both(lib, W, S, cells, commitments=commitments)
        assert got == want and got["ok"] == 0 and got["first_failing"] == -1 and got["rounds"] == 1, (got, want)
        got, want = both(lib, W, S, cells, commitments=commitments, locate=True)
        assert got == want and got["ok"] == 0 and got["first_failing"] == where and got["rounds"] >= 2, (where, got, want)
    got, want = both(lib, W, S, (which, cell, values, proofs))  # the next call is the honest one
    assert got == want and got["ok"] == 1


def test_points_off_the_curve_and_at_infinity(lib, oracle, worlds, tmp_path):
    """an off-curve commitment at index 200 of 257 beside an off-curve proof: a commitment comes before every cell; two in one wave of commitments and one
    in the last wave; then the zero polynomial, whose commitment and proofs are at infinity, under labels >= 64"""
    W = worlds(16, 4)
    S, count = 257, 300
    which, cell, values, proofs = cells_under(W, uniform(S, count))
    p2 = proofs.copy()
    p2[7] = off_curve(oracle, proofs[7])
    for spots in ((200,), (130, 190, 256)):
        cs = commitments_of(W, S)
        for c in spots:
            cs[c] = off_curve(oracle, cs[c])
        got, want = both(lib, W, S, (which, cell, values, proofs), commitments=cs, locate=True)
        assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=len(spots), first_bad=spots[0], first_bad_is_proof=0), got
        got, want = both(lib, W, S, (which, cell, values, p2), commitments=cs)
        assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=len(spots) + 1, first_bad=spots[0], first_bad_is_proof=0), got
    got, want = both(lib, W, S, (which, cell, values, p2))  # the proof alone
    assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=1, first_bad=7, first_bad_is_proof=1), got
    V = rows_world(W, 70)
    cs = V["commitments"].copy()
    cs[69] = off_curve(oracle, cs[69])
    got, want = both_cosets(lib, V, commitments=cs)
    assert got == want and scalars(got) == honest(70 * 4, ok=0, rounds=0, bad_points=1, first_bad=69, first_bad_is_proof=0), got
    rnd = oracle.random_scalars(0x5BEC, 8 * 16).reshape(8, 16, 4).copy()
    rnd[1] = 0
    Z = make_world(lib, oracle, tmp_path, 16, 4, 8, coeffs=rnd)
    assert np.array_equal(Z["commitments"][1], INF) and np.array_equal(Z["proofs"][1], np.tile(INF, (4, 1)))
    labels = uniform(S, count)
    assert ((labels % 8 == 1) & (labels >= 64)).sum() > 10
    got, want = both(lib, Z, S, cells_under(Z, labels))
    assert got == want and scalars(got) == honest(count), got
    got, want = both(lib, Z, S, cells_under(Z, np.full(100, 249)))  # every cell of the zero polynomial: nothing to sum
    assert got == want and scalars(got) == honest(100) and got["a"] == [int(v) for v in INF] and got["b"] == [int(v) for v in INF], got


@pytest.mark.parametrize("n,l,batch", [(8, 4, 65), (8, 4, 130), (128, 64, 65)])
def test_open_cosets_form(lib, oracle, worlds, n, l, batch):
    """rows of 8 polynomials at stride n and n + 5: the twin's report and the labelled form's through cosets_as_labelled; a false value in row 64 located"""
    V = rows_world(worlds(n, l), batch)
    m = n // l
    want = lib.kzg_check_cells_layout(*args_of(V, *cosets_as_labelled(V)), seed=SEED)
    for pad in (0, 5):
        buf, stride = padded(oracle, V, pad)
        got, twin = both_cosets(lib, V, values=buf, stride=stride)
        assert got == twin == want and scalars(got) == honest(batch * m), (pad, got, twin)
        k, j = m - 1, l - 1
        buf[64 * stride + k + m * j] = plus_one(oracle, buf[64 * stride + k + m * j])
        got, twin = both_cosets(lib, V, values=buf, stride=stride, locate=True)
        assert got == twin and got["ok"] == 0 and got["first_failing"] == 64 * m + k, (pad, got, twin)


def test_rows_longer_than_a_piece(lib, oracle, worlds):
    """(n, l) = (2048, 1): 2048 cells per row, two pieces each, over 66 rows"""
    V = rows_world(worlds(2048, 1), 66)
    got, twin = both_cosets(lib, V)
    assert got == twin and scalars(got) == honest(66 * 2048), (got, twin)


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def calls(lib, oracle, worlds, falsify=None, bad_commitment=False):
    """256 cells at l = 4 in both forms: under 70 commitments in the labelled form, 64 rows of n = 16 in the open-cosets form.  falsify: the cell whose
    first value is changed; bad_commitment: a commitment off the curve"""
    W = worlds(16, 4)
    S = 70
    which, cell, values, proofs = cells_under(W, uniform(S, 256))
    V = rows_world(W, 64)
    transforms = aligned_copy(V["values"].reshape(-1, 4))
    cs, rows = commitments_of(W, S), V["commitments"].copy()
    if falsify is not None:
        values[falsify * 4] = plus_one(oracle, values[falsify * 4])
        transforms[(falsify // 4) * 16 + falsify % 4] = plus_one(oracle, transforms[(falsify // 4) * 16 + falsify % 4])  # cell k = falsify mod 4, j = 0
    if bad_commitment:
        cs[66], rows[60] = off_curve(oracle, cs[66]), off_curve(oracle, rows[60])
    return {"labelled": lambda **kw: both(lib, W, S, (which, cell, values, proofs), commitments=cs, **kw),
            "open_cosets": lambda **kw: both_cosets(lib, V, values=transforms, commitments=rows, **kw)}


def test_funnel_counts_of_warm_calls(lib, oracle, worlds):
    """256 cells at l = 4 in each form: the counts of include/bbgpu.h, honest and with a finding among the commitments; the staging is counted"""
    for form, run in calls(lib, oracle, worlds).items():
        run()  # warm
        (got, want), st = counted(lib, run, WARM[form])  # the twin makes no HIP call: the counts are the device call's
        print("funnels of one warm layout call of 256 cells at l = 4,", form, st)
        assert got == want and got["ok"] == 1 and st == WARM[form], (form, st)
    for form, run in calls(lib, oracle, worlds, bad_commitment=True).items():
        (got, want), st = counted(lib, run, WARM_FINDING[form])
        assert got == want and got["bad_points"] == 1 and got["rounds"] == 0 and st == WARM_FINDING[form], (form, st)
    assert lib.memory_stats()["staging_bytes"] >= 256 * (64 + 4 * 64) + 70 * 64


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["labelled", "open_cosets"])
def test_injected_failures_leave_nothing_behind(lib, oracle, worlds, form, kind):
    """every site of the funnel `kind` that one warm layout call with LOCATE over a false cell passes (fold and MSM rounds included), failed once.  These
    are the library's injected error returns; nothing faults on the device.  Each failure is an error return with no MSM slot pending, the live
    allocations of before and a staging that does not grow, and the very next call gives the honest report."""
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


def test_seed_rules_and_determinism(lib, worlds):
    W = worlds(16, 4)
    S = 257
    a = args_of(W, *cells_under(W, uniform(S, 600)), commitments=commitments_of(W, S))
    runs = [lib.kzg_check_cells_layout(*a, seed=SEED) for _ in range(2)]
    assert runs[0] == runs[1] and runs[0]["ok"] == 1
    drawn = [lib.kzg_check_cells_layout(*a) for _ in range(2)]
    assert all(r["ok"] == 1 for r in drawn) and drawn[0]["seed"] != drawn[1]["seed"] and drawn[0]["a"] != drawn[1]["a"]
    assert lib.host_kzg_check_cells_layout(*a, seed=np.array(drawn[0]["seed"], dtype=np.uint64)) == drawn[0]
