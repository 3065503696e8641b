"""MSMs over tables whose points COLLIDE (-m gpu), end to end through every MSM entry, against a closed form.

Everywhere else in the suite the points are x^i G for a random x: n different points, so that no point ever meets itself or its negative in a
bucket, no two chunk partials of a bucket are equal and no bucket sum repeats.  Here the table is x^i G for x = 1 (every point is G), x = -1
(G, -G, G, ...), a 4th and an 8th root of unity (four / eight points, each with its negative) and x = 2, plus a table of G's followed by
-G's.  Points collide when they share a bucket, and the bucket is chosen by the scalar's digits, so which branch is reached is a property of
the (table, mix) pair (tests/colliding.py raw_scalars spells the pairs out):
  * x = 1 under one_value / alternating / halves: one or two buckets per window hold the whole table as copies of ONE point -- the accumulation's
    madd_ip doubles at the second entry of every chunk, all full chunks leave equal partials, every level of the merge trees (light, heavy-bucket
    with the workgroup tree, quad) is a doubling, and the bucket sums are multiples k G that repeat across windows (the same-x path of the quad
    addition in the row / column / segment folds and of the host tail).  No cancellation happens inside the accumulation for these;
  * x = -1, root4, root8 under one_value (and halves, random): a bucket holds points AND their negatives -- sums k P with small k inside a
    chunk, which double at k = +-1, cancel when k returns to 0 (a clean infinity stored as a partial when the chunk ends there) and restart from the
    flag; the merges get equal, opposite and infinite partials;
  * the G...G -G...-G table under one_value: runs of equal points, so whole chunks sum to c G and others to -c G -- opposite partials in the merges.
The order of the entries inside a bucket is the sort's business, so "by construction" above means: whatever that order is, the operands of every
addition in such a bucket are multiples of one point.  That in-chunk cancellation and restart are reached is shown by a mutation that forgets
the restart (see the pull request that added this file), not assumed.

x = 2 is the window-table case: rows of a window table are 2^off[w] P_i, so with P_i = 2^i G row (w, i) EQUALS row (0, i + off[w]) -- points of
different windows that share one bucket set collide, which no per-window mode can produce.  Which of them meet in one bucket depends on the
digits: these collisions occur in partials and merges by chance, not by construction.

Expected value: (sum s_i x^i mod r) G -- one big-integer sum and one scalar multiplication.  The oracle's Pippenger is asserted to agree with it
when a case is built (tests/colliding.py Tables.case), and the cases up to 4096 points are also checked against what the REFERENCE returned
(tests/golden/msm_colliding.json).  Every comparison is exact."""
import numpy as np
import pytest

from oracle.pyoracle import FQ, aligned_copy
from tests.colliding import MIXES, XS, Tables, same_point
from tests.util import limbs

pytestmark = pytest.mark.gpu

# the smallest sizes at which each path exists: 25 is the first size the shipped host threshold sends to the GPU, 200 has per-window bucket sets and
# chunks of a few entries, 1023 / 1024 / 1025 are the switch to window tables with both residues of n mod 8 (16-byte digit loads or not), 2051 is odd
# with more than one sort block, 4096 the reference fixture's largest, 16384 where the heavy-bucket merge takes the repeated scalars
SIZES = (25, 200, 1023, 1024, 1025, 2051, 4096, 16384)
TABLE_MODE_MIN = 1024


@pytest.fixture(scope="module")
def gpu():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.shutdown()


@pytest.fixture(scope="module")
def tables(oracle):
    return Tables(oracle)


@pytest.fixture(scope="module")
def reference_points(golden):
    return {(c["x"], c["mix"], c["n"]): c for c in golden("msm_colliding.json")["cases"]}


def _check(oracle, reference_points, got, want, key, what=""):
    assert same_point(got, want, oracle.const(FQ, "one")), (key, what, "infinity expected" if int(want[7]) >> 63 else "")
    ref = reference_points.get(key)
    if ref is not None:  # the cases the reference saw
        if ref.get("infinity"):
            assert int(got[7]) >> 63 == 1, (key, what)
        else:
            assert np.array_equal(got[0:4], limbs(ref["px"])) and np.array_equal(got[4:8], limbs(ref["py"])) and not int(got[7]) >> 63, (key, what)


def _own_table(table, n):
    """the first n rows at an address of their own: a prefix of a larger resident table would be served from that table, with ITS window size"""
    return aligned_copy(table[:2 * n])


def _release(gpu, tab, n):
    """drop the copy a host-pointer call registered on first sight (registering again returns that entry); returns whether it had window tables,
    None below the size at which tables are cached at all"""
    if n < TABLE_MODE_MIN:
        return None
    h = gpu.srs_register(tab)
    try:
        return gpu.srs_has_window_tables(h)
    finally:
        gpu.srs_release(h)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("xname", XS)
def test_pippenger_colliding(gpu, oracle, tables, reference_points, xname, n):
    """the host-pointer entry, every table, every mix, every size regime"""
    tab = _own_table(tables.points(xname)[1], n)
    try:
        for mix in MIXES:
            sc, want = tables.case(xname, mix, n)
            _check(oracle, reference_points, gpu.pippenger(sc, tab, n), want, (xname, mix, n))
    finally:
        had_tables = _release(gpu, tab, n)
    assert had_tables == (None if n < TABLE_MODE_MIN else True)


@pytest.mark.parametrize("n", (1024, 4096, 16384))
@pytest.mark.parametrize("xname", XS)
def test_pippenger_colliding_per_window_bucket_sets(gpu, oracle, tables, reference_points, xname, n):
    """the same without window tables: one bucket set per window at sizes that otherwise share one"""
    tab = _own_table(tables.points(xname)[1], n)
    gpu.set_precompute(False)
    try:
        for mix in MIXES:
            sc, want = tables.case(xname, mix, n)
            _check(oracle, reference_points, gpu.pippenger(sc, tab, n), want, (xname, mix, n), "no tables")
    finally:
        gpu.set_precompute(True)  # first: the module's library must not stay in this mode whatever the release does
        had_tables = _release(gpu, tab, n)
    assert had_tables is False


@pytest.mark.parametrize("n", (4096, 16384))
@pytest.mark.parametrize("xname", ("one", "minus_one", "two"))
def test_device_shares_of_colliding_msms_add_up(gpu, oracle, tables, reference_points, xname, n):
    """the resident entries: the whole MSM, then 2 and 4 window ranges, bucket-range shares and row ranges of it, each folded with g1_sum.  A share
    of such an MSM is often the point at infinity, and shares are equal or opposite to one another"""
    import torch
    tab = _own_table(tables.points(xname)[1], n)
    h = gpu.srs_register(tab)
    try:
        assert gpu.srs_has_window_tables(h)
        W = gpu.srs_num_windows(h, n)
        assert W >= 4
        for mix in ("one_value", "alternating", "halves", "random"):
            sc, want = tables.case(xname, mix, n)
            key = (xname, mix, n)
            d = torch.from_numpy(np.array(sc).view(np.int64)).cuda()
            _check(oracle, reference_points, gpu.msm_device(h, d.data_ptr(), n), want, key, "msm_device")
            for parts in (2, 4):
                wb = [W * r // parts for r in range(parts + 1)]
                got = gpu.g1_sum(np.stack([gpu.msm_device(h, d.data_ptr(), n, 0, a, b) for a, b in zip(wb[:-1], wb[1:])]))
                _check(oracle, reference_points, got, want, key, "%d window ranges" % parts)
                got = gpu.g1_sum(np.stack([gpu.msm_wait(gpu.msm_device_buckets_async(h, d.data_ptr(), n, r, parts)) for r in range(parts)]))
                _check(oracle, reference_points, got, want, key, "%d bucket shares" % parts)
                rb = [W * n * r // parts for r in range(parts + 1)]
                got = gpu.g1_sum(np.stack([gpu.msm_wait(gpu.msm_device_rows_async(h, d.data_ptr(), n, a, b)) for a, b in zip(rb[:-1], rb[1:])]))
                _check(oracle, reference_points, got, want, key, "%d row ranges" % parts)
    finally:
        gpu.srs_release(h)


def test_device_batch_of_colliding_msms(gpu, oracle, tables, reference_points):
    """three jobs with three different mixes in one batched pass that share the sort and the accumulation, over the all-equal table (every job's
    chunks double) and over G, -G, G, ... (one_value: both signs in one bucket, the chunks double, cancel and restart; this job ends at infinity)"""
    import torch
    n = 4096
    for xname in ("one", "minus_one"):
        tab = _own_table(tables.points(xname)[1], n)
        h = gpu.srs_register(tab)
        try:
            mixes = ("one_value", "zero_pm1", "random")
            dev = [torch.from_numpy(np.array(tables.case(xname, m, n)[0]).view(np.int64)).cuda() for m in mixes]
            got = gpu.msm_batch_wait(gpu.msm_device_batch_async(h, [d.data_ptr() for d in dev], n))
            for m, out in zip(mixes, got):
                _check(oracle, reference_points, out, tables.case(xname, m, n)[1], (xname, m, n), "batch")
        finally:
            gpu.srs_release(h)


@pytest.mark.parametrize("tables_on", (True, False), ids=("window-tables", "no-tables"))
@pytest.mark.parametrize("n", (1024, 4096, 16384))
def test_pippenger_runs_of_a_point_and_its_negative(gpu, oracle, n, tables_on):
    """h copies of G followed by n - h copies of -G under ONE scalar: a single bucket per window holds runs of equal points, so chunks sum to c G
    and to -c G and the merge trees add opposite partials (and, where a chunk straddles the turn, partials that cancelled on the way).  h = n / 2
    ends at infinity, h = n / 2 - 5 at -10 s G.  Expected: (h - (n - h)) s G; the oracle's Pippenger has to agree"""
    from oracle.pyoracle import to_int
    from tests.colliding import R, closed_form_point, to_limbs
    G = oracle.g1_one_affine()
    NG = G.copy()
    NG[4:8] = oracle.neg(FQ, G[4:8])
    s = to_int(oracle.random_scalars(0xC0111DE5 + n, 1)[0])
    sc = to_limbs([s] * n)
    gpu.set_precompute(tables_on)
    try:
        for h in (n // 2, n // 2 - 5):
            tab = oracle.point_table(aligned_copy(np.concatenate([np.tile(G, (h, 1)), np.tile(NG, (n - h, 1))])))
            want = closed_form_point(oracle, (2 * h - n) * s % R)
            assert np.array_equal(oracle.msm_affine(sc, tab, n), want), ("oracle.msm_affine disagrees with the closed form", n, h)
            try:
                got = gpu.pippenger(sc, tab, n)
            finally:
                had_tables = _release(gpu, tab, n)
            assert same_point(got, want, oracle.const(FQ, "one")), (n, h)
            assert had_tables == tables_on
    finally:
        gpu.set_precompute(True)


@pytest.mark.parametrize("xname", XS)
def test_pippenger_low_memory_colliding(gpu, oracle, tables, reference_points, xname):
    """the plain n-entry table (the reference's pippenger_low_memory convention): the library derives the endomorphism half itself"""
    n = 1025
    plain = aligned_copy(tables.points(xname)[0][:n])
    for mix in MIXES:
        sc, want = tables.case(xname, mix, n)
        _check(oracle, reference_points, gpu.pippenger_low_memory(sc, plain, n), want, (xname, mix, n), "plain table")
