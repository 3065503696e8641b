"""bbgpu_kzg_recover_cells on the GPU (-m gpu): the kernels of csrc/kzg_recover_cells.hip (k_recover_roots, k_recover_vanish with its LDS tiles and its
tree across lanes, k_recover_scatter, k_recover_divide, k_recover_tail) and the driver in capi.hip against the host twin bit for bit -- coefficients, transforms, report, and
the elements between the polynomials, which must stay as they were.  The twin itself is held to the original polynomial and to Lagrange interpolation by
tests/test_kzg_recover_cells_host.py.  Shapes, with m = n / l cells and mu of them missing:
  k_recover_vanish runs G = min(64, 2^18 / m) lanes per cell index and 256 threads per workgroup: m = 2 (half a workgroup), 4 (one), 8 (two) at G = 64;
  G = 64, 32, 16, 8, 4 at m = 2^12 .. 2^16 -- every width the bound m <= 2^16 leaves (G = 1 and 2 would need m >= 2^17);
  its LDS tile holds T = 256 roots (BbGpu.RECOVER_TILE): mu = T - 1, T, T + 1, 2 T + 1 at m = 1024, and mu = 0 and 1;
  l = 1 .. 64 at n = 64 l for the scatter's and the divide's index arithmetic; batch 1, 3 and 64 at n = 256; one larger shape, (2^16, 64), half missing;
  k_recover_tail runs at most 1024 workgroups of 256: (2^19, 64) takes it through a second trip, with extra coefficients whose index the report must name.
Then altered cells, a round trip through bbgpu_kzg_open_cosets_device and bbgpu_kzg_check_open_cosets, and the error contract under injected failures of
the four host-side funnels (no failure is provoked on the device)."""
import numpy as np
import pytest

from tests.kzg_recover_cells_cases import PAD, call_values, coefficient_buffer, memory, missing_sets, polynomial, present_cells

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
T = 256
TAIL = 1 << 18  # KZG_RECOVER_TAIL_MAX_BLOCKS = 1024 workgroups of 256: coefficient TAIL + i is thread i's second
# the funnels one warm call at (n, l) = (256, 4) with the transforms read back passes (include/bbgpu.h): allocations -- the cell lists, z and z', the values,
# the findings, the copy the forward transform works in; uploads -- the lists, the findings' start, the values; read-backs -- the findings, the transforms;
# launch checks -- k_recover_roots with k_recover_vanish, the batch inversion's two scans and its product, k_recover_scatter, four transforms, k_recover_divide, k_recover_tail
WARM = dict(alloc_calls=5, h2d_calls=3, d2h_calls=2, launch_checks=11)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    assert BbGpu.RECOVER_TILE == T
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def both(lib, n, l, d, cells, values, batch=1, pad=0, want_values=True):
    """the device call and the twin's over the same arguments, each into a buffer of the same other values -> ((buffer, transforms, report) x 2)"""
    import torch
    stride = n + pad
    buf = coefficient_buffer(batch, stride)
    d_out = dev(buf)
    got_v, got_rep = lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr(), batch=batch, stride=stride, want_values=want_values)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint64).reshape(-1, 4)
    want, want_v, want_rep = lib.host_kzg_recover_cells(cells, values, n, l, d, batch=batch, stride=stride, want_values=want_values, out=buf.copy())
    return (got, got_v, got_rep), (want, want_v, want_rep)


def agree(lib, n, l, d, missing, batch=1, pad=0, want_values=True, alter=None):
    cells = present_cells(n, l, missing)
    polys = [polynomial(n, d, b) for b in range(batch)]
    values = call_values([v for _, v in polys], n, l, cells)
    if alter is not None:
        values[alter] = memory([0xA17E2ED + alter])[0]  # row `alter` of the call's values: some other element
    (got, got_v, got_rep), (want, want_v, want_rep) = both(lib, n, l, d, cells, values, batch, pad, want_values)
    assert np.array_equal(got, want)
    assert (got_v is None and want_v is None and not want_values) or np.array_equal(got_v, want_v)
    assert got_rep == want_rep and got_rep["missing"] == len(missing)
    if alter is None:  # the twin's answer is the polynomial the cells came from
        rows = got.reshape(batch, n + pad, 4)
        for b, (c, _) in enumerate(polys):
            assert np.array_equal(rows[b, :n], memory(c)), b
        assert got_rep["consistent"] == 1
    return got_rep


def spread(m, mu, seed=3):
    return sorted(int(k) for k in np.random.default_rng([0x3B4D, m, mu, seed]).permutation(m)[:mu])


@pytest.mark.parametrize("m", [2, 4, 8])
def test_cell_counts_around_one_workgroup_of_the_vanishing_kernel(lib, m):
    for l in (1, 4):
        for mu in range(m):
            agree(lib, m * l, l, max(1, (m - mu) * l - 1), spread(m, mu), batch=2, pad=PAD)


@pytest.mark.parametrize("mu", [0, 1, T - 1, T, T + 1, 2 * T + 1])
def test_missing_counts_around_the_tile_of_roots(lib, mu):
    """m = 1024, l = 1: 64 lanes per cell index, four slices of a full tile each; mu = 2 T + 1 leaves one root in the third tile"""
    agree(lib, 1024, 1, 300, spread(1024, mu))


@pytest.mark.parametrize("log2m,lanes", [(12, 64), (13, 32), (14, 16), (15, 8), (16, 4)])
def test_every_width_of_the_lane_groups(lib, log2m, lanes):
    """l = 1; mu = 301 is no multiple of any width and spans two tiles"""
    assert lanes == min(64, (1 << 18) >> log2m)
    agree(lib, 1 << log2m, 1, 100, spread(1 << log2m, 301))


@pytest.mark.parametrize("l", [1, 2, 4, 8, 16, 32, 64])
def test_every_coset_size(lib, l):
    n = 64 * l
    for d, mu in ((n // 2, 32), (n // 2 + 1, 31), (max(1, l - 1), 63), (n, 0)):
        agree(lib, n, l, d, spread(64, mu), batch=2, pad=PAD)


@pytest.mark.parametrize("batch,pad,want_values", [(1, 0, True), (3, PAD, True), (3, PAD, False), (64, 0, True), (64, PAD, False)])
def test_batches_strides_and_the_optional_transforms(lib, batch, pad, want_values):
    for name, missing in missing_sets(256, 4, 100).items():
        agree(lib, 256, 4, 100, missing, batch=batch, pad=pad, want_values=want_values)


def test_a_larger_shape(lib):
    """(2^16, 64): 1024 cells, every even one missing, degree bound n / 2"""
    n, l = 1 << 16, 64
    agree(lib, n, l, n // 2, list(range(0, n // l, 2)))


@pytest.fixture(scope="module")
def big(lib, oracle):
    """(n, l) = (2^19, 64), batch 2, degree bound n / 4, 100 of the 8192 cells missing: polynomials and transforms by the device (bbgpu_ntt_device, which
    tests/test_gpu_ntt_sizes.py ties to the oracle), the cells, the listed values per polynomial.  Made once, never written to."""
    from tests.test_gpu_kzg_recover_each import cell_values, polynomials, split
    n, l, mu = 1 << 19, 64, 100
    coeffs, values = polynomials(lib, oracle, n, n // 4, 2, seed=7)
    cells = split(n // l, mu, 70)[1]
    return dict(n=n, l=l, d=n // 4, mu=mu, coeffs=coeffs, values=values, cells=cells, listed=[cell_values(values[b], l, cells) for b in range(2)])


def transforms_of(lib, coeffs):
    import torch
    t = dev(coeffs)
    lib.ntt_device(t.data_ptr(), coeffs.shape[0], "fft")
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def test_the_tail_past_its_grid(lib, big):
    """n = 2^19: the 1024 workgroups of 256 of k_recover_tail take a second trip.  Device against twin bit for bit (with mu = 100 the twin's products are
    few), the coefficients against the polynomials the cells were made from, the transforms against bbgpu_ntt_device's"""
    n, l, d = big["n"], big["l"], big["d"]
    (got, got_v, got_rep), (want, want_v, want_rep) = both(lib, n, l, d, big["cells"], np.concatenate(big["listed"]), batch=2, pad=PAD)
    assert np.array_equal(got, want) and np.array_equal(got_v, want_v)
    assert got_rep == want_rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, missing=big["mu"])
    assert np.array_equal(got.reshape(2, n + PAD, 4)[:, :n], big["coeffs"]) and np.array_equal(got_v, big["values"])


# coefficients of polynomial 1 beyond the degree bound 2^17 and below the (8192 - 100) x 64 values supplied: the cells then belong to a polynomial of
# degree below the number of values, which is recovered exactly, and the report names its first coefficient at or beyond the bound
EXTRA = {"last_of_trip_one": [TAIL - 1], "first_of_trip_two": [TAIL], "last_admissible": [(8192 - 100) * 64 - 1], "one_in_each_trip": [TAIL + 3, TAIL - 7]}


@pytest.mark.parametrize("where", sorted(EXTRA))
def test_the_tail_names_the_first_extra_coefficient(lib, big, where):
    import torch
    from tests.test_gpu_kzg_recover_each import cell_values
    n, l, d, cells = big["n"], big["l"], big["d"], big["cells"]
    assert all(d <= j < len(cells) * l for j in EXTRA[where])
    c1 = big["coeffs"][1].copy()
    for j in EXTRA[where]:
        c1[j] = memory([0xE17A + j])[0]
    v1 = transforms_of(lib, c1)
    d_out = dev(coefficient_buffer(2, n + PAD))
    got_v, rep = lib.kzg_recover_cells(cells, np.concatenate([big["listed"][0], cell_values(v1, l, cells)]), n, l, d, d_out.data_ptr(), batch=2, stride=n + PAD)
    torch.cuda.synchronize()
    rows = d_out.cpu().numpy().view(np.uint64).reshape(2, n + PAD, 4)
    assert rep == dict(consistent=0, first_bad_poly=1, first_bad_coeff=min(EXTRA[where]), missing=big["mu"])
    assert np.array_equal(rows[0, :n], big["coeffs"][0]) and np.array_equal(rows[1, :n], c1)
    assert np.array_equal(got_v[0], big["values"][0]) and np.array_equal(got_v[1], v1)


def test_one_altered_value_among_redundant_cells(lib):
    """batch 3 at (64, 16) and (256, 4), one value of polynomial 1 altered, count l > d: the device's report is the twin's, inconsistent, and names it"""
    for n, l, d, missing in ((64, 16, 17, [2]), (256, 4, 100, spread(64, 20))):
        count = n // l - len(missing)
        for spot in (0, count * l // 2, count * l - 1):
            rep = agree(lib, n, l, d, missing, batch=3, pad=PAD, alter=count * l + spot)
            assert rep["consistent"] == 0 and rep["first_bad_poly"] == 1 and d <= rep["first_bad_coeff"] < count * l


def test_three_polynomials_share_one_row_of_lists(lib):
    """(64, 4), m = 16: 9 cells listed out of order, 7 missing, batch 3 in a padded stride, degree bound 20, one value of polynomial 1 altered.  Scatter,
    divide and tail read every polynomial's lists, z and z' at a stride, which is zero for this entry: the smallest shape at which a stride that is not
    would take polynomial 1 or 2 to another row and show it.  Coefficients, transforms and report are the twin's (agree), which names polynomial 1."""
    n, l, d, missing = 64, 4, 20, spread(16, 7)
    cells = present_cells(n, l, missing)
    assert len(cells) == 9 and cells.tolist() != sorted(cells.tolist())
    rep = agree(lib, n, l, d, missing, batch=3, pad=PAD, alter=9 * l + 5)
    assert rep["consistent"] == 0 and rep["first_bad_poly"] == 1 and d <= rep["first_bad_coeff"] < 9 * l


def test_an_altered_value_without_redundancy_is_not_seen(lib):
    rep = agree(lib, 16, 4, 8, [0, 2], alter=3)
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, missing=2)


def test_round_trip_through_the_producer_and_the_checker(lib, oracle, tmp_path):
    """(256, 4), batch 2, degree < 128, 20 cells missing: the recovered coefficients go to bbgpu_kzg_open_cosets_device as they lie on the device; its
    proofs are the ones of the original polynomials, and bbgpu_kzg_check_open_cosets accepts the recovered transforms with them against the commitments of
    the ORIGINAL polynomials -- and rejects them after one recovered value is changed"""
    import torch
    from tests.kzg_check_cells_cases import SEED, cosets_args, make_world, plus_one, secret_x
    n, l, batch, d = 256, 4, 2, 128
    coeffs = oracle.random_scalars(0x2EC0, batch * n).reshape(batch, n, 4).copy()
    coeffs[:, d:] = 0
    W = make_world(lib, oracle, tmp_path, n, l, batch, coeffs=coeffs)
    cells = present_cells(n, l, spread(n // l, 20))
    values = np.ascontiguousarray(np.stack([W["values"][b, int(k)::n // l] for b in range(batch) for k in cells]).reshape(-1, 4))
    d_out = dev(coefficient_buffer(batch, n + PAD))
    got_v, rep = lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr(), batch=batch, stride=n + PAD)
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, missing=20) and np.array_equal(got_v, W["values"])
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


def warm_case():
    n, l, d = 256, 4, 100
    cells = present_cells(n, l, spread(64, 20))
    (c, v) = polynomial(n, d)
    return n, l, d, cells, call_values([v], n, l, cells), memory(c), memory(v)


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_funnel_counts_of_a_warm_call(lib):
    n, l, d, cells, values, want_c, want_v = warm_case()
    d_out = dev(np.zeros((n, 4), dtype=np.uint64))
    run = lambda: lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr())  # noqa: E731
    run()
    (got_v, rep), st = counted(lib, run, WARM)
    print("funnels of one warm call at (256, 4):", st)
    assert np.array_equal(got_v[0], want_v) and rep["consistent"] == 1 and st == WARM


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, kind):
    """every site of the funnel `kind` that one warm call at (256, 4) passes, failed once.  These are host-side funnels (the library's failure injection of
    API results); nothing faults on the device.  Each failure returns an error, leaves no allocation live, and the next call is bit-exact."""
    import torch
    from barretenberg_amd import BbGpuError
    n, l, d, cells, values, want_c, want_v = warm_case()
    d_out = dev(np.zeros((n, 4), dtype=np.uint64))

    def run():
        got_v, rep = lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr())
        torch.cuda.synchronize()
        return np.array_equal(got_v[0], want_v) and np.array_equal(d_out.cpu().numpy().view(np.uint64), want_c) and rep["consistent"] == 1
    assert run()  # warm
    _, sites = counted(lib, run, WARM)
    before = lib.fault_stats()
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
        assert run(), (kind, k)


def test_kernel_times_are_reported(lib):
    n, l, d, cells, values, _, _ = warm_case()
    d_out = dev(np.zeros((n, 4), dtype=np.uint64))
    lib.set_timing(1)
    try:
        lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr())
        with_values = lib.last_timing()
        lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr(), want_values=False)
        without = lib.last_timing()
    finally:
        lib.set_timing(0)
    # k_recover_vanish; scatter and IFFT; coset FFT, divide, coset IFFT and tail; the forward transform
    assert len(with_values) == 4 and len(without) == 3 and all(0 < v < 1000 for v in with_values + without), (with_values, without)
