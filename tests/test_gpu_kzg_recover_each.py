"""bbgpu_kzg_recover_cells_each on the GPU (-m gpu): the kernels of csrc/kzg_recover_each.hip (k_each_leaves, k_each_pair between the transforms of a tree
level, k_each_powers, k_each_gather), the back end it shares with bbgpu_kzg_recover_cells (k_recover_scatter, k_recover_divide, k_recover_tail of
csrc/kzg_recover_cells.hip, here with per-polynomial lists) and the driver in capi.hip
  against the host twin bit for bit -- coefficients with the elements between the polynomials, transforms, report, first_bad -- with one batch that holds
    mu_b = 0, 1, T - 1, T, T + 1, 2 T + 1 and m - 1 missing cells (T = BbGpu.RECOVER_EACH_LEAF roots per leaf: the edges of the leaf, of the padding with
    zero roots and of the first tree level), unsorted lists, the last polynomial without redundancy;
  against bbgpu_kzg_recover_cells bit for bit where every polynomial holds the same set;
  beyond that entry's 2^16 cells, where no twin is affordable, against the polynomials the cells were made from (values by bbgpu_ntt_device, which
    tests/test_gpu_ntt_sizes.py ties to the oracle), and once against the twin with few cells missing;
  past the grid of k_recover_tail (1024 workgroups of 256) at n = 2^19 and 2^20, with extra coefficients whose index the report must name exactly, and at
    batch x M = 2^22 roots, where the transforms of the first tree level are handed over in two chunks;
  a round trip through bbgpu_kzg_open_cosets_device and bbgpu_kzg_check_open_cosets; and the error contract under injected failures of the four host-side
  funnels (no failure is provoked on the device).  The twin itself is held to plain-integer interpolation by tests/test_kzg_recover_each_host.py."""
import numpy as np
import pytest

from tests.kzg_recover_cells_cases import PAD, coefficient_buffer, memory
from tests.kzg_recover_each_cases import NONE

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
TAIL = 1 << 18  # KZG_RECOVER_TAIL_MAX_BLOCKS = 1024 workgroups of 256: coefficient TAIL + i is thread i's second
# the funnels one warm call passes with the transforms read back (include/bbgpu.h).  Allocations: the lists, the tree, z with z' and the power table, the
# values, the findings, the copy the forward transform works in; uploads: the lists, the findings' start, the values; read-backs: the findings, the
# transforms.  Launch checks at (256, 4), where 64 cells make one leaf per polynomial and no level: k_each_leaves, k_each_powers with k_each_gather, the
# Z transforms, the batch inversion's two scans and its product, k_recover_scatter, four transforms, k_recover_divide, k_recover_tail.  At (1024, 1) with up to
# 200 cells missing (M = 256, two levels; transforms of 128 .. 1024 points are one launch each) every level adds three.
WARM = {(256, 4): dict(alloc_calls=6, h2d_calls=3, d2h_calls=2, launch_checks=13), (1024, 1): dict(alloc_calls=6, h2d_calls=3, d2h_calls=2, launch_checks=19)}


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def polynomials(lib, oracle, n, d, batch, seed=0):
    """(coefficients, values), (batch, n, 4) each: seeded polynomials of degree < d and their size-n transforms by bbgpu_ntt_device"""
    import torch
    coeffs = oracle.random_scalars(0x2EC1 + 977 * seed + n + d, batch * n).reshape(batch, n, 4).copy()
    coeffs[:, d:] = 0
    t = dev(coeffs.reshape(-1, 4))
    for b in range(batch):
        lib.ntt_device(t.data_ptr() + 32 * n * b, n, "fft")
    torch.cuda.synchronize()
    return coeffs, host(t).reshape(batch, n, 4).copy()


def split(m, mu, seed):
    """(missing ascending, present in a seeded shuffled order)"""
    p = np.random.default_rng([0x3B4F, m, mu, seed]).permutation(m).astype(np.uint32)
    return np.sort(p[:mu]), np.ascontiguousarray(p[mu:])


def cell_values(values, l, cells):
    """(count, l, 4): point j of listed cell t of one polynomial's (n, 4) transforms is entry cells[t] + m j"""
    return np.ascontiguousarray(values.reshape(l, -1, 4)[:, cells].transpose(1, 0, 2))


def both(lib, n, l, d, cells, values, pad=0):
    """the device call and the twin's over the same arguments, each into a buffer of the same other values -> ((buffer, transforms, report, first_bad) x 2)"""
    import torch
    batch, stride = len(cells), n + pad
    buf = coefficient_buffer(batch, stride)
    d_out = dev(buf)
    got_v, got_rep, got_first = lib.kzg_recover_cells_each(cells, values, n, l, d, d_out.data_ptr(), stride=stride)
    torch.cuda.synchronize()
    want, want_v, want_rep, want_first = lib.host_kzg_recover_cells_each(cells, values, n, l, d, stride=stride, out=buf.copy())
    return (host(d_out), got_v, got_rep, got_first), (want, want_v, want_rep, want_first)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("n,l", [(2048, 1), (4096, 4), (1 << 16, 64)])
def test_device_equals_twin_around_the_leaf_and_the_first_level(lib, oracle, n, l):
    from barretenberg_amd import BbGpu
    T, m, d = BbGpu.RECOVER_EACH_LEAF, n // l, l  # degree bound l: every mu < m is admitted, and mu = m - 1 leaves no redundancy
    mus = [0, 1, T - 1, T, T + 1, 2 * T + 1, m - 1]
    assert all(mu < m for mu in mus) and (m - mus[-1]) * l == d
    coeffs, values = polynomials(lib, oracle, n, d, len(mus))
    cells = [split(m, mu, b)[1] for b, mu in enumerate(mus)]
    vals = [cell_values(values[b], l, c) for b, c in enumerate(cells)]
    got, want = both(lib, n, l, d, cells, vals, PAD)
    assert same(got, want)
    rows = got[0].reshape(len(mus), n + PAD, 4)
    assert np.array_equal(rows[:, :n], coeffs) and np.array_equal(got[1], values)
    assert got[2] == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=m - 1) and got[3].tolist() == [NONE] * len(mus)
    # one value of polynomials 4 and 6 altered: polynomial 4 (mu = T + 1) has redundancy and shows, polynomial 6 has none
    for b in (4, 6):
        vals[b] = vals[b].copy()
        vals[b][0, 0] = memory([0xA17E2ED + b])[0]
    got, want = both(lib, n, l, d, cells, vals, PAD)
    assert same(got, want)
    assert got[2]["consistent"] == 0 and got[2]["first_bad_poly"] == 4 and d <= got[2]["first_bad_coeff"] < (m - mus[4]) * l
    assert got[3].tolist() == [NONE] * 4 + [got[2]["first_bad_coeff"], NONE, NONE]


def test_neighbouring_polynomials_each_with_its_own_row(lib, oracle):
    """(64, 4), m = 16: batch 3 with 16, 9 and 5 cells listed (mu = 0, 7, 11, so M = 16 is below the leaf), degree bound 20.  One call in which the count
    of present values, mu and the row of missing cells all differ between neighbouring values of blockIdx.y of the shared scatter, divide and tail
    (csrc/kzg_recover_cells.hip), and one polynomial has no missing cell at all.  Device against twin bit for bit, first_bad included."""
    n, l, d, mus = 64, 4, 20, (0, 7, 11)
    coeffs, values = polynomials(lib, oracle, n, d, len(mus), seed=8)
    cells = [split(n // l, mu, 90 + b)[1] for b, mu in enumerate(mus)]
    assert [len(c) for c in cells] == [16, 9, 5]
    got, want = both(lib, n, l, d, cells, [cell_values(values[b], l, c) for b, c in enumerate(cells)], PAD)
    assert same(got, want)
    assert np.array_equal(got[0].reshape(len(mus), n + PAD, 4)[:, :n], coeffs) and np.array_equal(got[1], values)
    assert got[2] == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=11) and got[3].tolist() == [NONE] * len(mus)


@pytest.mark.parametrize("n,l,batch,mu", [(1 << 12, 64, 4, None), (1 << 16, 1, 1, 300)])
def test_device_equals_the_same_set_entry(lib, oracle, n, l, batch, mu):
    """every polynomial holds the same cells: coefficients, transforms and verdict are bbgpu_kzg_recover_cells's, bit for bit"""
    import torch
    m, d = n // l, n // 4
    if mu is None:
        missing, cells = np.arange(0, m, 2, dtype=np.uint32), np.random.default_rng(5).permutation(np.arange(1, m, 2, dtype=np.uint32))
    else:
        missing, cells = split(m, mu, 9)
    coeffs, values = polynomials(lib, oracle, n, d, batch, seed=1)
    vals = [cell_values(values[b], l, cells) for b in range(batch)]
    buf = coefficient_buffer(batch, n + PAD)
    d_old, d_new = dev(buf), dev(buf)
    old_v, old_rep = lib.kzg_recover_cells(cells, np.concatenate(vals), n, l, d, d_old.data_ptr(), batch=batch, stride=n + PAD)
    new_v, new_rep, first = lib.kzg_recover_cells_each([cells] * batch, vals, n, l, d, d_new.data_ptr(), stride=n + PAD)
    torch.cuda.synchronize()
    assert np.array_equal(host(d_new), host(d_old)) and np.array_equal(new_v, old_v) and np.array_equal(new_v, values)
    assert new_rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=len(missing)) and old_rep["missing"] == len(missing)
    assert old_rep["consistent"] == 1 and first.tolist() == [NONE] * batch


@pytest.mark.parametrize("log2n", [17, 18])
def test_beyond_the_cell_limit_of_the_same_set_entry(lib, oracle, log2n):
    """l = 1, batch 2, two different random sets with about half the cells missing and an odd mu, degree bound n / 4: the recovered coefficients are the
    original ones, the transforms those of bbgpu_ntt_device; then one value of polynomial 1 altered"""
    import torch
    n, l, batch = 1 << log2n, 1, 2
    d, mus = n // 4, [n // 2 - 1, n // 2 - 1001]
    coeffs, values = polynomials(lib, oracle, n, d, batch, seed=2)
    cells = [split(n, mu, 20 + b)[1] for b, mu in enumerate(mus)]
    vals = [cell_values(values[b], l, c) for b, c in enumerate(cells)]
    d_out = dev(np.zeros((batch * n, 4), dtype=np.uint64))
    got_v, rep, first = lib.kzg_recover_cells_each(cells, vals, n, l, d, d_out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(host(d_out).reshape(batch, n, 4), coeffs) and np.array_equal(got_v, values)
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=max(mus)) and first.tolist() == [NONE, NONE]
    vals[1] = vals[1].copy()
    vals[1][12345, 0] = memory([0xA17E2ED])[0]
    _, rep, first = lib.kzg_recover_cells_each(cells, vals, n, l, d, d_out.data_ptr(), want_values=False)
    torch.cuda.synchronize()
    assert rep["consistent"] == 0 and rep["first_bad_poly"] == 1 and d <= rep["first_bad_coeff"] < len(cells[1])
    assert first.tolist() == [NONE, rep["first_bad_coeff"]] and np.array_equal(host(d_out).reshape(batch, n, 4)[0], coeffs[0])


def test_device_equals_twin_beyond_the_cell_limit(lib, oracle):
    """n = 2^17, l = 1, mu = (T + 1, 3): few enough missing cells for the twin's direct products"""
    from barretenberg_amd import BbGpu
    n, l, d = 1 << 17, 1, 1 << 15
    mus = [BbGpu.RECOVER_EACH_LEAF + 1, 3]
    coeffs, values = polynomials(lib, oracle, n, d, 2, seed=3)
    cells = [split(n, mu, 30 + b)[1] for b, mu in enumerate(mus)]
    got, want = both(lib, n, l, d, cells, [cell_values(values[b], l, c) for b, c in enumerate(cells)])
    assert same(got, want) and np.array_equal(got[0].reshape(2, n, 4), coeffs) and got[2]["consistent"] == 1 and got[2]["max_missing"] == mus[0]


def transforms_of(lib, coeffs):
    import torch
    t = dev(coeffs)
    lib.ntt_device(t.data_ptr(), coeffs.shape[0], "fft")
    torch.cuda.synchronize()
    return host(t)


@pytest.fixture(scope="module")
def big(lib, oracle):
    """(n, l) = (2^19, 64), batch 2, degree bound n / 4, 100 and 37 of the 8192 cells missing.  Made once, never written to."""
    n, l, mus = 1 << 19, 64, (100, 37)
    coeffs, values = polynomials(lib, oracle, n, n // 4, 2, seed=5)
    cells = [split(n // l, mu, 60 + b)[1] for b, mu in enumerate(mus)]
    return dict(n=n, l=l, d=n // 4, mus=mus, coeffs=coeffs, values=values, cells=cells, vals=[cell_values(values[b], l, c) for b, c in enumerate(cells)])


def test_the_tail_past_its_grid(lib, big):
    """n = 2^19: the 1024 workgroups of 256 of k_recover_tail take a second trip.  Device against twin bit for bit (few cells are missing, so the twin's
    direct products are few), the coefficients against the original polynomials, the transforms against bbgpu_ntt_device's"""
    n = big["n"]
    got, want = both(lib, n, big["l"], big["d"], big["cells"], big["vals"], PAD)
    assert same(got, want)
    assert np.array_equal(got[0].reshape(2, n + PAD, 4)[:, :n], big["coeffs"]) and np.array_equal(got[1], big["values"])
    assert got[2] == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=100) and got[3].tolist() == [NONE, NONE]


# coefficients of polynomial 1 beyond the degree bound 2^17 and below the (8192 - 37) x 64 values it supplies: its cells then belong to a polynomial of
# degree below the number of values, which is recovered exactly, and the report names its first coefficient at or beyond the bound
EXTRA = {"last_of_trip_one": [TAIL - 1], "first_of_trip_two": [TAIL], "last_admissible": [(8192 - 37) * 64 - 1], "one_in_each_trip": [TAIL + 3, TAIL - 7]}


@pytest.mark.parametrize("where", sorted(EXTRA))
def test_the_tail_names_the_first_extra_coefficient(lib, big, where):
    import torch
    n, l, d, cells = big["n"], big["l"], big["d"], big["cells"]
    assert all(d <= j < len(cells[1]) * l for j in EXTRA[where])
    c1 = big["coeffs"][1].copy()
    for j in EXTRA[where]:
        c1[j] = memory([0xE17A + j])[0]
    v1 = transforms_of(lib, c1)
    d_out = dev(coefficient_buffer(2, n + PAD))
    got_v, rep, first = lib.kzg_recover_cells_each(cells, [big["vals"][0], cell_values(v1, l, cells[1])], n, l, d, d_out.data_ptr(), stride=n + PAD)
    torch.cuda.synchronize()
    rows = host(d_out).reshape(2, n + PAD, 4)
    assert rep == dict(consistent=0, first_bad_poly=1, first_bad_coeff=min(EXTRA[where]), max_missing=100) and first.tolist() == [NONE, min(EXTRA[where])]
    assert np.array_equal(rows[0, :n], big["coeffs"][0]) and np.array_equal(rows[1, :n], c1)
    assert np.array_equal(got_v[0], big["values"][0]) and np.array_equal(got_v[1], v1)


@pytest.fixture(scope="module")
def huge(lib, oracle):
    """(n, l, batch) = (2^20, 1, 4), degree bound n / 4, 2^19 + 1, 0, 65 and 1000 points missing: the common padded count is M = 2^20, so the first tree
    level transforms batch x M / 64 = 65,536 slots of 128 points -- two chunks of the 32768 that recover_each_ntt (capi.hip) hands over at a time.  Made
    once, never written to."""
    n, mus = 1 << 20, ((1 << 19) + 1, 0, 65, 1000)
    coeffs, values = polynomials(lib, oracle, n, n // 4, 4, seed=6)
    cells = [split(n, mu, 80 + b)[1] for b, mu in enumerate(mus)]
    return dict(n=n, d=n // 4, mus=mus, coeffs=coeffs, values=values, cells=cells, vals=[cell_values(values[b], 1, c) for b, c in enumerate(cells)])


def test_the_chunk_loop_of_the_tree_transforms(lib, huge):
    """batch x M = 2^22: no twin at this size (its direct products would be 2^39).  The recovered coefficients are the original polynomials, all four in
    full, the transforms bbgpu_ntt_device's, the report consistent with max_missing = 2^19 + 1"""
    import torch
    n = huge["n"]
    d_out = dev(np.zeros((4 * n, 4), dtype=np.uint64))
    got_v, rep, first = lib.kzg_recover_cells_each(huge["cells"], huge["vals"], n, 1, huge["d"], d_out.data_ptr())
    torch.cuda.synchronize()
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=(1 << 19) + 1) and first.tolist() == [NONE] * 4
    assert np.array_equal(host(d_out).reshape(4, n, 4), huge["coeffs"]) and np.array_equal(got_v, huge["values"])


def test_the_fourth_trip_of_the_tail(lib, huge):
    """the same call with an extra coefficient of polynomial 2 at 3 x 2^18 + 5 (k_recover_tail's fourth trip at n = 2^20) and one of polynomial 3 at 2^18,
    the degree bound itself: the first findings per polynomial, and the report names polynomial 2"""
    import torch
    n, extra = huge["n"], {2: 3 * TAIL + 5, 3: TAIL}
    coeffs, vals = huge["coeffs"].copy(), list(huge["vals"])
    for b, j in extra.items():
        assert huge["d"] <= j < len(huge["cells"][b])
        coeffs[b, j] = memory([0xE17A + j])[0]
        vals[b] = cell_values(transforms_of(lib, coeffs[b]), 1, huge["cells"][b])
    d_out = dev(np.zeros((4 * n, 4), dtype=np.uint64))
    _, rep, first = lib.kzg_recover_cells_each(huge["cells"], vals, n, 1, huge["d"], d_out.data_ptr(), want_values=False)
    torch.cuda.synchronize()
    assert rep == dict(consistent=0, first_bad_poly=2, first_bad_coeff=extra[2], max_missing=(1 << 19) + 1)
    assert first.tolist() == [NONE, NONE, extra[2], extra[3]]
    assert np.array_equal(host(d_out).reshape(4, n, 4), coeffs)  # polynomials 0 and 1 the originals, 2 and 3 with their extra terms


def test_round_trip_through_the_producer_and_the_checker(lib, oracle, tmp_path):
    """(4096, 64), batch 2, degree < 2048, 20 and 7 cells missing: the recovered coefficients go to bbgpu_kzg_open_cosets_device as they lie on the device;
    its proofs are those of the original polynomials and bbgpu_kzg_check_open_cosets accepts the recovered transforms with them against the commitments
    of the ORIGINAL polynomials -- and rejects them after one recovered value is changed"""
    import torch
    from tests.kzg_check_cells_cases import SEED, cosets_args, make_world, plus_one, secret_x
    n, l, batch, d = 4096, 64, 2, 2048
    coeffs = oracle.random_scalars(0x2EC2, batch * n).reshape(batch, n, 4).copy()
    coeffs[:, d:] = 0
    W = make_world(lib, oracle, tmp_path, n, l, batch, coeffs=coeffs)
    cells = [split(n // l, mu, 40 + b)[1] for b, mu in enumerate((20, 7))]
    vals = [cell_values(W["values"][b], l, c) for b, c in enumerate(cells)]
    d_out = dev(coefficient_buffer(batch, n + PAD))
    got_v, rep, first = lib.kzg_recover_cells_each(cells, vals, n, l, d, d_out.data_ptr(), stride=n + PAD)
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=20) and np.array_equal(got_v, W["values"])
    h = lib.srs_generate(secret_x(oracle), n)
    try:
        setup = lib.kzg_open_cosets_setup(h, n, l)
        try:
            proofs = lib.kzg_open_cosets_device(setup, d_out.data_ptr(), n, l, batch=batch, stride=n + PAD)
            torch.cuda.synchronize()
        finally:
            lib.kzg_open_cosets_release(setup)
    finally:
        lib.srs_release(h)
    assert np.array_equal(proofs, W["proofs"])
    flat = np.ascontiguousarray(got_v.reshape(-1, 4))
    assert lib.kzg_check_open_cosets(*cosets_args(W, values=flat, proofs=proofs), seed=SEED)["ok"] == 1
    flat[n + 77] = plus_one(oracle, flat[n + 77])
    assert lib.kzg_check_open_cosets(*cosets_args(W, values=flat, proofs=proofs), seed=SEED)["ok"] == 0


_warm = {}


def warm_case(lib, oracle, n, l):
    """batch 2 with different sets; at (1024, 1) 200 and 70 cells missing, which makes two tree levels"""
    if (n, l) not in _warm:
        m, d = n // l, n // 4
        coeffs, values = polynomials(lib, oracle, n, d, 2, seed=4)
        cells = [split(m, mu, 50 + b)[1] for b, mu in enumerate((20, 9) if m == 64 else (200, 70))]
        _warm[(n, l)] = (d, cells, [cell_values(values[b], l, c) for b, c in enumerate(cells)], coeffs.reshape(-1, 4), values)
    return _warm[(n, l)]


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


@pytest.mark.parametrize("n,l", sorted(WARM))
def test_funnel_counts_of_a_warm_call(lib, oracle, n, l):
    d, cells, vals, want_c, want_v = warm_case(lib, oracle, n, l)
    d_out = dev(np.zeros((2 * n, 4), dtype=np.uint64))
    run = lambda: lib.kzg_recover_cells_each(cells, vals, n, l, d, d_out.data_ptr())  # noqa: E731
    run()
    (got_v, rep, _), st = counted(lib, run, WARM[(n, l)])
    print("funnels of one warm call at", (n, l), st)
    assert np.array_equal(got_v, want_v) and rep["consistent"] == 1 and st == WARM[(n, l)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,l", sorted(WARM))
def test_injected_failures_leave_nothing_behind(lib, oracle, n, l, kind):
    """every site of the funnel `kind` that one warm call passes, failed once.  These are host-side funnels (the library's failure injection of API
    results); nothing faults on the device.  Each failure returns BBGPU_ERR_HIP, leaves no allocation live, and the next call is bit-exact."""
    import torch
    from barretenberg_amd import BbGpuError
    d, cells, vals, want_c, want_v = warm_case(lib, oracle, n, l)
    d_out = dev(np.zeros((2 * n, 4), dtype=np.uint64))

    def run():
        got_v, rep, first = lib.kzg_recover_cells_each(cells, vals, n, l, d, d_out.data_ptr())
        torch.cuda.synchronize()
        return np.array_equal(got_v, want_v) and np.array_equal(host(d_out), want_c) and rep["consistent"] == 1 and first.tolist() == [NONE, NONE]
    assert run()  # warm
    _, sites = counted(lib, run, WARM[(n, l)])
    before, held = lib.fault_stats(), lib.memory_stats()
    for k in range(sites[KEYS[kind]] + 1):  # k == sites: the armed failure no longer fires
        lib.fault_inject("%s:%d" % (kind, k))
        if k < sites[KEYS[kind]]:
            with pytest.raises(BbGpuError, match=" -1:"):
                run()
            st = lib.fault_stats()
            assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        else:
            assert run(), (kind, k)
            st = lib.fault_stats()
            assert st["fired"] == 0 and st["armed"] == 1, (kind, k, st)
        lib.fault_inject(None)
        torch.cuda.synchronize()
        st = lib.fault_stats()
        assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        assert lib.memory_stats() == held, (kind, k)
        assert run(), (kind, k)


def test_kernel_times_are_reported(lib, oracle):
    n, l = 1024, 1
    d, cells, vals, _, _ = warm_case(lib, oracle, n, l)
    d_out = dev(np.zeros((2 * n, 4), dtype=np.uint64))
    lib.set_timing(1)
    try:
        lib.kzg_recover_cells_each(cells, vals, n, l, d, d_out.data_ptr())
        with_values = lib.last_timing()
        lib.kzg_recover_cells_each(cells, vals, n, l, d, d_out.data_ptr(), want_values=False)
        without = lib.last_timing()
    finally:
        lib.set_timing(0)
    # the tree and the Z transforms; scatter and IFFT; coset FFT, divide, coset IFFT and tail; the forward transform
    assert len(with_values) == 4 and len(without) == 3 and all(0 < v < 1000 for v in with_values + without), (with_values, without)
