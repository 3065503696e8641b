"""The bucket accumulation (msm_accumulate_kernel) at the edges of its loop: entry lists shorter than, equal to and one past a chunk
and a workgroup, negative digits at every position of a chunk, long runs of empty buckets, one-bucket lists, and shares whose range ends
inside a chunk.  Every result is compared, bit for bit, with BbGpu.host_msm on the same inputs: the library's separate host bucket code,
which tests/test_host_fallback.py pins to the reference's fixtures.  Inputs are seeded splitmix64 streams as in bench.py."""
import numpy as np
import pytest

from tests.util import SCALAR_SEED, SRS_SEED

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1000, 4099, (1 << 16) + 3]
BIG = (1 << 19) + 3  # window tables of 2^19 < n <= 2^20 points: the 15-window layout of the 2^20 headline
SKEW_SIZES = [4099, (1 << 16) + 3]
SIGN_N = 4099
SCALAR_BITS = 254


@pytest.fixture(scope="module")
def G():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    g.set_host_thresholds(0, 0)  # every size on the GPU kernels
    yield g
    g.set_precompute(True)
    g.shutdown()


@pytest.fixture(scope="module")
def x_secret():
    import bench
    x_raw = bench.raw_scalars(1, SRS_SEED)[0]
    return bench.limbs_of(sum(int(v) << (64 * i) for i, v in enumerate(x_raw)) * (1 << 256) % bench.FR_MODULUS)


@pytest.fixture(scope="module")
def uniform(G):
    """bench.py's scalar stream, in Montgomery form, once for the largest size (every case takes a prefix)"""
    import bench
    import torch
    return bench.to_montgomery_on_device(G, bench.raw_scalars(BIG, SCALAR_SEED), torch.device("cuda:0")).cpu().numpy().view(np.uint64).reshape(BIG, 4)


class Cases:
    """host tables and host results, computed once and shared by the two table modes"""

    def __init__(self, G, x):
        self.G, self.x, self.tables, self.wants = G, x, {}, {}

    def table(self, n):
        if n not in self.tables:
            h, t = self.G.srs_generate(self.x, n, want_host_table=True)
            self.G.srs_release(h)
            self.tables[n] = t
        return self.tables[n]

    def want(self, key, scalars, n):
        if key not in self.wants:
            self.wants[key] = self.G.host_msm(np.ascontiguousarray(scalars[:n]), self.table(n), n)
        return self.wants[key]


@pytest.fixture(scope="module")
def cases(G, x_secret):
    return Cases(G, x_secret)


def same_point(got, want):
    inf_g, inf_w = int(got[7]) >> 63, int(want[7]) >> 63
    return inf_g == inf_w and (inf_w == 1 or np.array_equal(got[:8], want[:8]))


def device_msm(G, x, scalars, n, tables):
    import torch
    G.set_precompute(tables)
    h = G.srs_generate(x, n)
    d = torch.from_numpy(np.ascontiguousarray(scalars[:n]).view(np.int64)).cuda()
    try:
        return G.msm_device(h, d.data_ptr(), n)
    finally:
        G.srs_release(h)


@pytest.mark.parametrize("tables", [True, False], ids=["window-tables", "no-tables"])
@pytest.mark.parametrize("n", SIZES)
def test_entry_lists_around_a_chunk_and_a_workgroup(G, x_secret, uniform, cases, n, tables):
    """n windows-many entries: from one lane with fewer entries than a chunk (n = 1) over lists that fill a chunk, a wave and a workgroup
    exactly, by one less and by one more, to many workgroups"""
    assert same_point(device_msm(G, x_secret, uniform, n, tables), cases.want(("uniform", n), uniform, n)), n


def test_entry_list_of_the_15_window_layout(G, x_secret, uniform, cases):
    """2^19 + 3 points against window tables: 15 windows of 17 bits, the layout of the 2^20-point headline, with a ragged end"""
    G.set_precompute(True)
    h = G.srs_generate(x_secret, BIG)
    layout = (G.srs_has_window_tables(h), G.srs_num_windows(h, BIG))
    G.srs_release(h)
    assert layout == (True, 15)
    assert same_point(device_msm(G, x_secret, uniform, BIG, True), cases.want(("uniform", BIG), uniform, BIG))


def sign_pattern_scalars(G, n, c, pattern):
    """Raw scalars whose signed c-bit digits have a chosen sign whatever carry arrives from below: a window value in [2^(c-1) + 1, 2^c - 2]
    gives a negative digit, one in [1, 2^(c-1) - 2] a positive one.  Patterns:
      neg      every digit negative (the carry out of the last full window is the one positive digit of a scalar): the first, the last and every
               entry of every chunk is negative
      alt      points alternate all-negative / all-positive: every other entry of a bucket's run (entries of a bucket keep the order of the points)
      neg_one  as neg with ONE window value for all points and windows: one bucket, chunks of nothing but negative entries, first to last
      alt_one  as alt on that one bucket (and its positive twin): every other entry negative through whole chunks"""
    import bench
    import torch
    full = (SCALAR_BITS - 4) // c  # windows filled; the value stays below 2^250 < r
    half = 1 << (c - 1)
    hi_span, lo_span = (1 << c) - 2 - (half + 1) + 1, half - 2
    r = bench.splitmix64(0x51695EED00000000 + c, n * full).reshape(n, full)
    hi = (half + 1) + (r % np.uint64(hi_span)).astype(np.int64)
    lo = 1 + (r % np.uint64(lo_span)).astype(np.int64)
    if pattern.endswith("_one"):
        hi[:], lo[:] = half + 1 + hi_span // 3, 1 + lo_span // 3
    negative = np.ones(n, dtype=bool) if pattern.startswith("neg") else (np.arange(n) % 2 == 0)
    vals = np.where(negative[:, None], hi, lo)
    raw = np.zeros((n, 4), dtype=np.uint64)
    for i in range(n):
        v = 0
        for w in range(full):
            v |= int(vals[i, w]) << (c * w)
        raw[i] = bench.limbs_of(v)
    return bench.to_montgomery_on_device(G, raw, torch.device("cuda:0")).cpu().numpy().view(np.uint64).reshape(n, 4)


@pytest.mark.parametrize("tables", [True, False], ids=["window-tables", "no-tables"])
@pytest.mark.parametrize("pattern", ["neg", "alt", "neg_one", "alt_one"])
def test_negative_digits_at_every_position_of_a_chunk(G, x_secret, cases, pattern, tables):
    """see sign_pattern_scalars.  The window size is the table's (or the size rule's without tables) and known here only through the number
    of windows, so every window size with that number of windows gets its own vector: one of them is the layout meant, the others are
    valid inputs all the same"""
    n = SIGN_N
    G.set_precompute(tables)
    h = G.srs_generate(x_secret, n)
    W = G.srs_num_windows(h, n)
    G.srs_release(h)
    sizes = [c for c in range(4, 21) if SCALAR_BITS // c + 1 == W]
    assert sizes, W
    for c in sizes:
        sc = sign_pattern_scalars(G, n, c, pattern)
        assert same_point(device_msm(G, x_secret, sc, n, tables), cases.want((pattern, c), sc, n)), (pattern, c)


@pytest.mark.parametrize("tables", [True, False], ids=["window-tables", "no-tables"])
@pytest.mark.parametrize("n", SKEW_SIZES)
@pytest.mark.parametrize("kind", ["zero_one", "small", "all_equal"])
def test_empty_bucket_runs_and_one_bucket_lists(G, x_secret, cases, kind, n, tables):
    """bench.skewed_scalars: scalars in {0, 1, -1} and below 200 leave a handful of full buckets between long runs of empty ones (the
    search that skips them, the dummy bucket past the end of the list); equal scalars put every window's entries into one bucket"""
    import bench
    sc = bench.skewed_scalars(kind, n)
    assert same_point(device_msm(G, x_secret, sc, n, tables), cases.want((kind, n), sc, n)), (kind, n)


def test_shares_that_end_inside_a_chunk(G, x_secret, uniform, cases):
    """a row-range share and a bucket-range share of one 2^16 + 3 point MSM whose ranges end at no boundary of anything (an odd row inside
    a window; a third of the bucket range): the accumulation's last lane of each share stops inside its chunk and walks on into the dummy
    bucket.  The shares fold to the full result"""
    import torch
    n = (1 << 16) + 3
    want = cases.want(("uniform", n), uniform, n)
    G.set_precompute(True)
    h = G.srs_generate(x_secret, n)
    d = torch.from_numpy(np.ascontiguousarray(uniform[:n]).view(np.int64)).cuda()
    try:
        R = G.srs_num_windows(h, n) * n
        cut = (R * 3) // 8 + 1
        parts = [G.msm_wait(G.msm_device_rows_async(h, d.data_ptr(), n, a, b)) for a, b in ((0, cut), (cut, R))]
        assert same_point(G.g1_sum(np.stack(parts)), want)
        parts = [G.msm_wait(G.msm_device_buckets_async(h, d.data_ptr(), n, r, 3)) for r in range(3)]
        assert same_point(G.g1_sum(np.stack(parts)), want)
    finally:
        G.srs_release(h)
