"""bbgpu_kzg_open_cosets_setup_bounded with bbgpu_kzg_open_cosets_device on the GPU (-m gpu): the kernels of csrc/kzg_open_cosets.hip where the degree bound
d is below n -- strings, scalars and ladders at size M = 2 d / l, the replicating gather, the forward stages from log2 (m / mu) on -- against the host twin
bit for bit (itself held to the quotient definition by tests/test_kzg_open_bounded_host.py; it runs every stage over the zero-padded input), against an
unbounded setup on the device, and through the chain the entry is for.  Shapes (n, l, d): (8, 2, 4) mu = 2, M = 4, a partly filled wave, rho = 2;
(16, 1, 4) no tree, rho = 4: two replicated levels; (256, 64, 128) a full-wave tree with mu = 2; (512, 4, 256) M = 128, the first size with the
groups-per-wave addressing of k_lagrange_stage, sixteen frequencies per wave; (1024, 64, 128) rho = 8; (1024, 1, 4) m > d: the proofs outgrow the
scalars' buffer; (4096, 64, 2048) new against old."""
import numpy as np
import pytest

from oracle.pyoracle import aligned_copy
from tests.kzg_open_bounded_cases import (ERR_ARG, ERR_SIZE, ERR_STATE, INF, PAD, bounded_reference, buffer_of, coset_polynomials, extended, secret_x)

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
ROWS = 4096
WARM_SHAPE = (512, 4, 256)
# the funnels one warm call at (n, l, d) = (512, 4, 256) passes (include/bbgpu.h): allocations -- the scalars' buffer (later the proofs) and the scratch
# points; no upload; read-backs -- the proofs (one staging chunk); launch checks -- k_open_cosets_t, the transform of the four t^(e) of length 128 (one
# group, one pass), the chain from the sum kernel to the finish kernel.  A warm setup: S^; the curve findings up and down; the curve pass and the chain of
# the string kernel and the stages.  They are the counts of an unbounded setup at (256, 4): the same M.
WARM = dict(alloc_calls=2, h2d_calls=0, d2h_calls=1, launch_checks=3)
WARM_SETUP = dict(alloc_calls=1, h2d_calls=1, d2h_calls=1, launch_checks=2)


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


@pytest.fixture(scope="module")
def world(lib, oracle):
    """the generated table of a known x (handle and host copy), one setup per (n, l, d), and per (n, l, d) the host twin's proofs of every case polynomial
    of length d (one twin call each): made once, never written to.  reset() after a bbgpu_shutdown: the handle and the setups are gone with it."""
    W = dict(setups={}, twins={})

    def reset():
        W["setups"].clear()
        W["h"], W["table"] = lib.srs_generate(secret_x(oracle), ROWS, want_host_table=True)

    def setup(n, l, d):
        if (n, l, d) not in W["setups"]:
            W["setups"][(n, l, d)] = lib.kzg_open_cosets_setup(W["h"], n, l, degree_bound=d)
        return W["setups"][(n, l, d)]

    def twin(n, l, d):
        if (n, l, d) not in W["twins"]:
            cases = coset_polynomials(oracle, d, l)
            got = lib.host_kzg_open_cosets(aligned_copy(W["table"][:2 * d]), n, l, buffer_of(oracle, [c for _, c in cases], d), batch=len(cases), degree_bound=d)
            W["twins"][(n, l, d)] = {name: got[k] for k, (name, _) in enumerate(cases)}
        return W["twins"][(n, l, d)]
    reset()
    W.update(setup=setup, twin=twin, reset=reset)
    yield W
    for s in W["setups"].values():
        lib.kzg_open_cosets_release(s)


def open_bounded(lib, setup, polys, n, l, stride, oracle):
    """one device call over the polynomials `polys` (d coefficients each) at `stride`, other values between them; the input on the device is unchanged
    afterwards"""
    import torch
    buf = buffer_of(oracle, polys, stride)
    d = dev(buf)
    got = lib.kzg_open_cosets_device(setup, d.data_ptr(), n, l, batch=len(polys), stride=stride)
    torch.cuda.synchronize()
    assert got.shape == (len(polys), n // l, 8) and np.array_equal(d.cpu().numpy().view(np.uint64), buf)
    return got


@pytest.mark.parametrize("n,l,d", [(8, 2, 4), (16, 1, 4), (256, 64, 128), (512, 4, 256), (1024, 64, 128), (1024, 1, 4)])
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, PAD)])
def test_device_against_twin(lib, oracle, world, n, l, d, batch, pad):
    """every case polynomial of length d, `batch` of them per call (the list wraps) at stride d + pad, bit for bit"""
    cases, want = coset_polynomials(oracle, d, l), world["twin"](n, l, d)
    for k in range(0, len(cases), batch):
        group = [cases[(k + b) % len(cases)] for b in range(batch)]
        got = open_bounded(lib, world["setup"](n, l, d), [c for _, c in group], n, l, d + pad, oracle)
        for b, (name, _) in enumerate(group):
            assert np.array_equal(got[b], want[name]), (name, b)
    if l > 1:
        for name in ("degree < l", "last level cancels"):
            assert np.array_equal(want[name], np.tile(INF, (n // l, 1))), name
    assert lib.fault_stats()["slots_pending"] == 0


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_a_bound_of_n_is_the_setup_without_one(lib, oracle, world):
    """(256, 4, 256): the proofs of bbgpu_kzg_open_cosets_setup bit for bit, its footprint (2 n x 128 bytes) and its funnel counts"""
    from barretenberg_amd import BbGpuError
    from tests.test_gpu_kzg_open_cosets import WARM as OLD_WARM, WARM_SETUP as OLD_WARM_SETUP
    n, l = 256, 4
    polys = [c for _, c in coset_polynomials(oracle, n, l)]
    old = lib.kzg_open_cosets_setup(world["h"], n, l)
    try:
        want = open_bounded(lib, old, polys, n, l, n + PAD, oracle)
    finally:
        lib.kzg_open_cosets_release(old)
    before = lib.memory_stats()
    s, st = counted(lib, lambda: lib.kzg_open_cosets_setup(world["h"], n, l, degree_bound=n), OLD_WARM_SETUP)
    try:
        assert st == OLD_WARM_SETUP
        assert lib.memory_stats() == dict(before, staging_bytes=before["staging_bytes"] + 2 * n * 128)
        assert np.array_equal(open_bounded(lib, s, polys, n, l, n + PAD, oracle), want)
        got, st = counted(lib, lambda: open_bounded(lib, s, polys[:1], n, l, n, oracle), OLD_WARM)
        assert st == OLD_WARM and np.array_equal(got[0], want[0])
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_device(s, 0x1000, n, l, stride=n - 1)
    finally:
        lib.kzg_open_cosets_release(s)
    assert lib.memory_stats() == before


def test_new_against_old_at_a_larger_size(lib, oracle, world):
    """(4096, 64, 2048), batch 2, random coefficients: all 64 cosets equal those of an unbounded setup over the zero-padded coefficients; eight fixed cosets
    of each polynomial, the first and the last among them, also against synthetic division and bbgpu_host_msm_g1"""
    n, l, d, batch = 4096, 64, 2048, 2
    m = n // l
    c = aligned_copy(oracle.random_scalars(0x4096B0, batch * d))
    polys = [c[b * d:(b + 1) * d] for b in range(batch)]
    got = open_bounded(lib, world["setup"](n, l, d), polys, n, l, d, oracle)
    old = lib.kzg_open_cosets_setup(world["h"], n, l)
    try:
        zero_padded = dev(np.concatenate([extended(p, n) for p in polys]))
        assert np.array_equal(got, lib.kzg_open_cosets_device(old, zero_padded.data_ptr(), n, l, batch=batch))
    finally:
        lib.kzg_open_cosets_release(old)
    picks = [0, m - 1, 1, m // 2, 5, 22, 43, m - 2]
    for b in range(batch):
        assert np.array_equal(got[b][picks], bounded_reference(lib, oracle, world["table"], polys[b], n, l, cosets=picks)), b


def test_polynomials_back_to_back(lib, oracle, world):
    """(512, 4, 256), batch 3, stride == d: polynomial b + 1 starts where the coefficients of polynomial b end"""
    n, l, d = WARM_SHAPE
    cases, want = coset_polynomials(oracle, d, l)[:3], world["twin"](n, l, d)
    got = open_bounded(lib, world["setup"](n, l, d), [c for _, c in cases], n, l, d, oracle)
    for b, (name, _) in enumerate(cases):
        assert np.array_equal(got[b], want[name]), name


def test_a_table_of_d_rows_opens_on_the_domain_of_twice_its_size(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    n, l, d = WARM_SHAPE
    h = lib.srs_generate(secret_x(oracle), d)
    try:
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_setup(h, n, l)
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_setup(h, 4 * n, l, degree_bound=2 * d)
        s = lib.kzg_open_cosets_setup(h, n, l, degree_bound=d)
    finally:
        lib.srs_release(h)  # the setup does not read the table again
    try:
        name, c = coset_polynomials(oracle, d, l)[0]
        assert np.array_equal(open_bounded(lib, s, [c], n, l, d, oracle)[0], world["twin"](n, l, d)[name])
    finally:
        lib.kzg_open_cosets_release(s)


def test_a_row_off_the_curve_is_named_and_rows_from_d_minus_l_on_are_not_read(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    from tests.srs_update_cases import tampered
    n, l, d = 128, 4, 64
    h = lib.srs_register(tampered(tampered(world["table"][:2 * n], 37), 41))
    try:
        live = lib.fault_stats()["live_allocations"]
        with pytest.raises(BbGpuError, match=ERR_ARG + ".*row 37 "):
            lib.kzg_open_cosets_setup(h, n, l, degree_bound=d)
        assert lib.fault_stats()["live_allocations"] == live
    finally:
        lib.srs_release(h)
    h = lib.srs_register(tampered(tampered(tampered(world["table"][:2 * n], d - l), d), n - 1))
    try:
        lib.kzg_open_cosets_release(lib.kzg_open_cosets_setup(h, n, l, degree_bound=d))
    finally:
        lib.srs_release(h)


def test_the_chain_it_is_for(lib, oracle, world, tmp_path):
    """(256, 4, 128): half of the 64 cells of a degree-< 128 polynomial are dropped, bbgpu_kzg_recover_cells leaves the coefficients on the device, and a
    bounded open reads them there with that call's stride: the proofs are the twin's proofs of the original polynomial, bbgpu_kzg_check_open_cosets accepts
    them against the original commitment, and rejects them once one proof is swapped for another"""
    import torch
    from tests.kzg_check_cells_cases import SEED, cosets_args, make_world
    from tests.kzg_recover_cells_cases import coefficient_buffer, present_cells
    n, l, d = 256, 4, 128
    m = n // l
    coeffs = oracle.random_scalars(0xB0C4A1, n).reshape(1, n, 4).copy()
    coeffs[:, d:] = 0
    W = make_world(lib, oracle, tmp_path, n, l, 1, coeffs=coeffs)
    missing = sorted(int(k) for k in np.random.default_rng([0xB0C4A1, m]).permutation(m)[:m // 2])
    cells = present_cells(n, l, missing)
    values = np.ascontiguousarray(np.stack([W["values"][0, int(k)::m] for k in cells]).reshape(-1, 4))
    stride = n + PAD
    d_out = dev(coefficient_buffer(1, stride))
    got_v, rep = lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr(), stride=stride)
    assert rep == dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, missing=m // 2) and np.array_equal(got_v, W["values"])
    proofs = lib.kzg_open_cosets_device(world["setup"](n, l, d), d_out.data_ptr(), n, l, stride=stride)
    torch.cuda.synchronize()
    want = lib.host_kzg_open_cosets(aligned_copy(world["table"][:2 * d]), n, l, aligned_copy(coeffs[0, :d]), degree_bound=d)
    assert np.array_equal(proofs, want) and np.array_equal(proofs, W["proofs"])
    flat = np.ascontiguousarray(got_v.reshape(-1, 4))
    assert lib.kzg_check_open_cosets(*cosets_args(W, values=flat, proofs=proofs), seed=SEED)["ok"] == 1
    swapped = proofs.copy()
    swapped[0, 9] = proofs[0, 10]
    assert not np.array_equal(swapped, proofs)
    assert lib.kzg_check_open_cosets(*cosets_args(W, values=flat, proofs=swapped), seed=SEED)["ok"] == 0


def test_setup_memory_is_counted_and_returned(lib, oracle, world):
    """setup, call, release and setup again leave bbgpu_memory_stats where it was; the 2 d rows of S^ are counted in staging_bytes while the setup lives"""
    n, l, d = WARM_SHAPE
    name, c = coset_polynomials(oracle, d, l)[0]
    s = lib.kzg_open_cosets_setup(world["h"], n, l, degree_bound=d)  # warm: the staging of the curve findings and of the transform is grown
    open_bounded(lib, s, [c], n, l, d, oracle)
    lib.kzg_open_cosets_release(s)
    before, live = lib.memory_stats(), lib.fault_stats()
    for _ in range(2):
        s = lib.kzg_open_cosets_setup(world["h"], n, l, degree_bound=d)
        during = lib.memory_stats()
        assert during == dict(before, staging_bytes=before["staging_bytes"] + 2 * d * 128)
        assert lib.fault_stats()["live_allocations"] == live["live_allocations"] + 1
        assert np.array_equal(open_bounded(lib, s, [c], n, l, d, oracle)[0], world["twin"](n, l, d)[name])
        assert lib.memory_stats() == during
        lib.kzg_open_cosets_release(s)
        after = lib.fault_stats()
        assert lib.memory_stats() == before and after["live_allocations"] == live["live_allocations"] and after["live_bytes"] == live["live_bytes"]


def test_funnel_counts_of_warm_calls(lib, oracle, world):
    n, l, d = WARM_SHAPE
    name, c = coset_polynomials(oracle, d, l)[0]
    lib.kzg_open_cosets_release(lib.kzg_open_cosets_setup(world["h"], n, l, degree_bound=d))  # warm
    s, st = counted(lib, lambda: lib.kzg_open_cosets_setup(world["h"], n, l, degree_bound=d), WARM_SETUP)
    lib.kzg_open_cosets_release(s)
    print("funnels of one warm setup at (512, 4, 256):", st)
    assert st == WARM_SETUP
    run = lambda: open_bounded(lib, world["setup"](n, l, d), [c], n, l, d, oracle)[0]  # noqa: E731
    run()
    got, st = counted(lib, run, WARM)
    print("funnels of one warm call at (512, 4, 256):", st)
    assert np.array_equal(got, world["twin"](n, l, d)[name]) and st == WARM


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, oracle, world, kind):
    """every site of the funnel `kind` that one warm call at (512, 4, 256) passes, failed once.  These are host-side funnels (the library's failure
    injection of API results); nothing faults on the device.  Each failure returns BBGPU_ERR_HIP, leaves no allocation live and staging_bytes where it was,
    and the next call over the same setup is bit-exact.  The same over a warm bounded setup: after a failed one no setup exists."""
    import torch
    from barretenberg_amd import BbGpuError
    n, l, d = WARM_SHAPE
    name, c = coset_polynomials(oracle, d, l)[0]
    want = world["twin"](n, l, d)[name]
    s = world["setup"](n, l, d)
    dc = dev(c)
    run = lambda: lib.kzg_open_cosets_device(s, dc.data_ptr(), n, l, stride=d)[0]  # noqa: E731
    assert np.array_equal(run(), want)  # warm
    before, staging = lib.fault_stats(), lib.memory_stats()["staging_bytes"]
    for k in range(WARM[KEYS[kind]] + 1):  # k == sites: the armed failure no longer fires
        lib.fault_inject("%s:%d" % (kind, k))
        if k < WARM[KEYS[kind]]:
            with pytest.raises(BbGpuError, match=" -1:"):
                run()
            st = lib.fault_stats()
            assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        else:
            assert np.array_equal(run(), want), (kind, k)
            st = lib.fault_stats()
            assert st["fired"] == 0 and st["armed"] == 1, (kind, k, st)
        lib.fault_inject(None)
        torch.cuda.synchronize()
        st = lib.fault_stats()
        assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        assert lib.memory_stats()["staging_bytes"] == staging, (kind, k)
        assert np.array_equal(run(), want), (kind, k)  # the setup stays usable
    for k in range(WARM_SETUP[KEYS[kind]]):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError, match=" -1:"):
            lib.kzg_open_cosets_setup(world["h"], n, l, degree_bound=d)
        st = lib.fault_stats()
        lib.fault_inject(None)
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"] and st["slots_pending"] == 0, (kind, k, st)
        assert lib.memory_stats()["staging_bytes"] == staging, (kind, k)
    s2 = lib.kzg_open_cosets_setup(world["h"], n, l, degree_bound=d)
    assert np.array_equal(lib.kzg_open_cosets_device(s2, dc.data_ptr(), n, l, stride=d)[0], want)
    lib.kzg_open_cosets_release(s2)


def test_argument_errors_on_a_bound_device(lib, oracle, world):
    """the verdicts that need a table or a setup; bounded and unbounded setups share one pool of BBGPU_KZG_OPEN_COSETS_MAX_SETUPS"""
    from barretenberg_amd import BbGpuError
    fake = 0x1000  # never dereferenced
    with pytest.raises(BbGpuError, match=ERR_SIZE):  # d above the table
        lib.kzg_open_cosets_setup(world["h"], 1 << 14, 64, degree_bound=2 * ROWS)
    n, l, d = WARM_SHAPE
    s = world["setup"](n, l, d)
    for kw in (dict(stride=d - 1), dict(stride=0), dict(batch=0, stride=d), dict(batch=65, stride=d)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_device(s, fake, n, l, **kw)
    big = lib.kzg_open_cosets_setup(world["h"], 1 << 16, 64, degree_bound=ROWS)  # the batch rule is that of the domain: batch x 2 n <= 2^22
    try:
        for batch in (33, 64):
            with pytest.raises(BbGpuError, match=ERR_SIZE):
                lib.kzg_open_cosets_device(big, fake, 1 << 16, 64, batch=batch, stride=ROWS)
        live = lib.fault_stats()["live_allocations"]
        taken = []
        with pytest.raises(BbGpuError, match=ERR_STATE):
            for k in range(17):
                taken.append(lib.kzg_open_cosets_setup(world["h"], 8, 2, degree_bound=4) if k % 2 else lib.kzg_open_cosets_setup(world["h"], 4, 2))
        assert 1 <= len(taken) <= 15 and lib.fault_stats()["live_allocations"] == live + len(taken)
        for bound in (None, 4):
            with pytest.raises(BbGpuError, match=ERR_STATE):
                lib.kzg_open_cosets_setup(world["h"], 8, 2, degree_bound=bound)
        lib.kzg_open_cosets_release(taken.pop())
        taken.append(lib.kzg_open_cosets_setup(world["h"], 8, 2, degree_bound=4))
        for t in taken:
            lib.kzg_open_cosets_release(t)
        assert lib.fault_stats()["live_allocations"] == live
    finally:
        lib.kzg_open_cosets_release(big)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kzg_open_cosets_device(big, fake, 1 << 16, 64, stride=ROWS)


def test_kernel_times_are_reported(lib, oracle, world):
    n, l, d = WARM_SHAPE
    lib.set_timing(1)
    try:
        open_bounded(lib, world["setup"](n, l, d), [coset_polynomials(oracle, d, l)[0][1]], n, l, d, oracle)
        ms = lib.last_timing()
    finally:
        lib.set_timing(0)
    assert len(ms) == 4 and all(0 < v < 1000 for v in ms), ms  # the sum kernel, the inverse stages, the gather and the forward stages, the finish kernel


def test_shutdown_releases_the_setups(lib, oracle, world):
    """bbgpu_shutdown frees every bounded setup with its rows: the handles are unknown afterwards, and a new start finds the pool empty"""
    from barretenberg_amd import BbGpuError
    s = world["setup"](8, 2, 4)
    extra = lib.kzg_open_cosets_setup(world["h"], 16, 1, degree_bound=4)
    lib.shutdown()
    try:
        assert lib.fault_stats()["live_allocations"] == 0
        for dead in (s, extra):
            with pytest.raises(BbGpuError, match=ERR_ARG):
                lib.kzg_open_cosets_release(dead)
            with pytest.raises(BbGpuError, match=ERR_ARG):
                lib.kzg_open_cosets_device(dead, 0x1000, 8, 2, stride=4)
    finally:
        world["reset"]()  # the next call binds the device again
    taken = [lib.kzg_open_cosets_setup(world["h"], 8, 2, degree_bound=4) for _ in range(16)]
    for t in taken:
        lib.kzg_open_cosets_release(t)
    name, c = coset_polynomials(oracle, 4, 2)[0]
    assert np.array_equal(open_bounded(lib, world["setup"](8, 2, 4), [c], 8, 2, 4, oracle)[0], world["twin"](8, 2, 4)[name])
