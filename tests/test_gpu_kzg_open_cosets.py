"""bbgpu_kzg_open_cosets_setup / bbgpu_kzg_open_cosets_device on the GPU (-m gpu): the kernels of csrc/kzg_open_cosets.hip (the l strings and their
transforms, the scalars of t^(e), the sum kernel with its ladders and its tree of additions across lanes, both group transforms over a batch, the gather, the
normalisation with infinities) against the host twin bit for bit -- itself held to the quotient definition by tests/test_kzg_open_cosets_host.py -- against
the definition directly at a larger size, and against the fold of bbgpu_kzg_open_all_device's own proofs.  Sizes (n, l): (4, 2) a partly filled wave and
M = 4; (2, 1) and (64, 1) no tree, also bbgpu_kzg_open_all_device bit for bit (two entries with a pool each over one device path); (8, 4); (128, 64) a full-wave tree over the shortest transform; (256, 4)
sixteen frequencies per wave, M = 128 the first size with the groups-per-wave addressing of k_lagrange_stage; (256, 64), at batch 3 with 192 scalar
transforms: more than one group of 64; (4096, 64) against the definition."""
import numpy as np
import pytest

from oracle.pyoracle import aligned_copy
from tests.kzg_open_cosets_cases import (ERR_ARG, ERR_SIZE, ERR_STATE, INF, PAD, buffer_of, coset_polynomials, fold_single_proofs, infinite_row_table, polynomials,
                                         reference, secret_x)

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
ROWS = 4096
# the funnels one warm call at (n, l) = (256, 4) passes (include/bbgpu.h): allocations -- t (later the proofs) and the scratch points; no upload; read-backs
# -- the proofs (one staging chunk); launch checks -- k_open_cosets_t, the transform of the four t^(e) (one group), the chain from the sum kernel to the
# finish kernel.  A warm setup: S^; the curve findings up and down; the curve pass and the chain of the string kernel and the stages.
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
    """the generated table of a known x (handle and host copy), one setup per (n, l), and per (n, l) the host twin's proofs of every case polynomial (one
    twin call each): made once, never written to.  reset() after a bbgpu_shutdown: the handle and the setups are gone with it."""
    W = dict(setups={}, twins={})

    def reset():
        W["setups"].clear()
        W["h"], W["table"] = lib.srs_generate(secret_x(oracle), ROWS, want_host_table=True)

    def setup(n, l):
        if (n, l) not in W["setups"]:
            W["setups"][(n, l)] = lib.kzg_open_cosets_setup(W["h"], n, l)
        return W["setups"][(n, l)]

    def twin(n, l):
        if (n, l) not in W["twins"]:
            cases = coset_polynomials(oracle, n, l)
            got = lib.host_kzg_open_cosets(aligned_copy(W["table"][:2 * n]), n, l, buffer_of(oracle, [c for _, c in cases], n), batch=len(cases))
            W["twins"][(n, l)] = {name: got[k] for k, (name, _) in enumerate(cases)}
        return W["twins"][(n, l)]
    reset()
    W.update(setup=setup, twin=twin, reset=reset)
    yield W
    for s in W["setups"].values():
        lib.kzg_open_cosets_release(s)


def open_cosets(lib, setup, polys, n, l, stride, oracle):
    """one device call over the polynomials `polys`; the input on the device is unchanged afterwards"""
    import torch
    buf = buffer_of(oracle, polys, stride)
    d = dev(buf)
    got = lib.kzg_open_cosets_device(setup, d.data_ptr(), n, l, batch=len(polys), stride=stride)
    torch.cuda.synchronize()
    assert got.shape == (len(polys), n // l, 8) and np.array_equal(d.cpu().numpy().view(np.uint64), buf)
    return got


@pytest.mark.parametrize("n,l,batch,pad", [(4, 2, 1, 0), (4, 2, 3, PAD), (2, 1, 1, 0), (2, 1, 3, PAD), (64, 1, 1, 0), (64, 1, 3, PAD), (8, 4, 1, 0), (8, 4, 3, PAD),
                                           (128, 64, 1, 0), (128, 64, 3, PAD), (256, 4, 1, 0), (256, 4, 3, PAD), (256, 64, 1, 0), (256, 64, 3, PAD)])
def test_device_against_twin(lib, oracle, world, n, l, batch, pad):
    """every case polynomial, `batch` of them per call (the list wraps), bit for bit; at l = 1 also bbgpu_kzg_open_all_device's proofs: the same kernels
    reached through the other entry and the other pool"""
    cases, want = coset_polynomials(oracle, n, l), world["twin"](n, l)
    for k in range(0, len(cases), batch):
        group = [cases[(k + b) % len(cases)] for b in range(batch)]
        got = open_cosets(lib, world["setup"](n, l), [c for _, c in group], n, l, n + pad, oracle)
        for b, (name, _) in enumerate(group):
            assert np.array_equal(got[b], want[name]), (name, b)
    if l > 1:
        for name in ("degree < l", "last level cancels"):
            assert np.array_equal(want[name], np.tile(INF, (n // l, 1))), name
    else:
        single = lib.kzg_open_all_setup(world["h"], n)
        try:
            d = dev(buffer_of(oracle, [c for _, c in cases], n + pad))
            assert np.array_equal(lib.kzg_open_cosets_device(world["setup"](n, 1), d.data_ptr(), n, 1, batch=len(cases), stride=n + pad),
                                  lib.kzg_open_all_device(single, d.data_ptr(), n, batch=len(cases), stride=n + pad))
        finally:
            lib.kzg_open_all_release(single)
    assert lib.fault_stats()["slots_pending"] == 0


def test_a_larger_size_against_the_definition(lib, oracle, world):
    """(4096, 64), batch 2, random coefficients: eight fixed cosets of each polynomial, the first and the last among them, against synthetic division and
    bbgpu_host_msm_g1"""
    n, l, batch = 4096, 64, 2
    m = n // l
    c = aligned_copy(oracle.random_scalars(0x4096C0, batch * n))
    got = open_cosets(lib, world["setup"](n, l), [c[b * n:(b + 1) * n] for b in range(batch)], n, l, n, oracle)
    picks = [0, m - 1, 1, m // 2, 5, 22, 43, m - 2]
    for b in range(batch):
        assert np.array_equal(got[b][picks], reference(lib, oracle, world["table"], c[b * n:(b + 1) * n], l, cosets=picks)), b


def test_device_against_the_fold_of_its_own_single_proofs(lib, oracle, world):
    """(256, 4): pi_k = sum_j [omega^(k + m j) / (l psi^k)] pi(omega^(k + m j)) over bbgpu_kzg_open_all_device's proofs of the same polynomial"""
    n, l = 256, 4
    c = coset_polynomials(oracle, n, l)[0][1]
    single = lib.kzg_open_all_setup(world["h"], n)
    try:
        singles = lib.kzg_open_all_device(single, dev(c).data_ptr(), n)[0]
    finally:
        lib.kzg_open_all_release(single)
    assert np.array_equal(open_cosets(lib, world["setup"](n, l), [c], n, l, n, oracle)[0], fold_single_proofs(lib, oracle, singles, n, l))


@pytest.mark.parametrize("l", [1, 2])
def test_a_string_whose_transform_has_a_row_at_infinity(lib, oracle, l):
    """x = W zeta at n = 4: row 1 of DFT_8 of the whole string is the point at infinity (l = 1); at l = 2 the same table through two strings of one row"""
    table = infinite_row_table(oracle)
    h = lib.srs_register(table)
    try:
        setup = lib.kzg_open_cosets_setup(h, 4, l)
        try:
            cases = polynomials(oracle, 4)
            want = lib.host_kzg_open_cosets(table, 4, l, buffer_of(oracle, [c for _, c in cases], 4), batch=len(cases))
            assert np.array_equal(open_cosets(lib, setup, [c for _, c in cases], 4, l, 4, oracle), want)
        finally:
            lib.kzg_open_cosets_release(setup)
    finally:
        lib.srs_release(h)


def test_a_row_off_the_curve_is_named_and_no_setup_is_made(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    from tests.srs_update_cases import tampered
    n, l = 64, 4
    h = lib.srs_register(tampered(tampered(world["table"][:2 * n], 37), 41))
    try:
        live = lib.fault_stats()["live_allocations"]
        with pytest.raises(BbGpuError, match=ERR_ARG + ".*row 37 "):
            lib.kzg_open_cosets_setup(h, n, l)
        assert lib.fault_stats()["live_allocations"] == live
    finally:
        lib.srs_release(h)
    h = lib.srs_register(tampered(tampered(world["table"][:2 * n], n - l), n - 1))  # rows from n - l on are not read
    try:
        lib.kzg_open_cosets_release(lib.kzg_open_cosets_setup(h, n, l))
    finally:
        lib.srs_release(h)


def test_setup_memory_is_counted_and_returned(lib, oracle, world):
    """setup, call, release and setup again leave bbgpu_memory_stats where it was; the 2 n rows of S^ are counted in staging_bytes while the setup lives"""
    n, l = 256, 4
    c = coset_polynomials(oracle, n, l)[0][1]
    s = lib.kzg_open_cosets_setup(world["h"], n, l)  # warm: the staging of the curve findings and of the transform is grown
    open_cosets(lib, s, [c], n, l, n, oracle)
    lib.kzg_open_cosets_release(s)
    before, live = lib.memory_stats(), lib.fault_stats()
    for _ in range(2):
        s = lib.kzg_open_cosets_setup(world["h"], n, l)
        during = lib.memory_stats()
        assert during == dict(before, staging_bytes=before["staging_bytes"] + 2 * n * 128)
        assert lib.fault_stats()["live_allocations"] == live["live_allocations"] + 1
        assert np.array_equal(open_cosets(lib, s, [c], n, l, n, oracle)[0], world["twin"](n, l)["random"])
        assert lib.memory_stats() == during
        lib.kzg_open_cosets_release(s)
        after = lib.fault_stats()
        assert lib.memory_stats() == before and after["live_allocations"] == live["live_allocations"] and after["live_bytes"] == live["live_bytes"]


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_funnel_counts_of_warm_calls(lib, oracle, world):
    n, l = 256, 4
    c = coset_polynomials(oracle, n, l)[0][1]
    lib.kzg_open_cosets_release(lib.kzg_open_cosets_setup(world["h"], n, l))  # warm
    s, st = counted(lib, lambda: lib.kzg_open_cosets_setup(world["h"], n, l), WARM_SETUP)
    lib.kzg_open_cosets_release(s)
    print("funnels of one warm setup at (256, 4):", st)
    assert st == WARM_SETUP
    run = lambda: open_cosets(lib, world["setup"](n, l), [c], n, l, n, oracle)[0]  # noqa: E731
    run()
    got, st = counted(lib, run, WARM)
    print("funnels of one warm call at (256, 4):", st)
    assert np.array_equal(got, world["twin"](n, l)["random"]) and st == WARM


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, oracle, world, kind):
    """every site of the funnel `kind` that one warm call at (256, 4) passes, failed once.  These are host-side funnels (the library's failure injection of
    API results); nothing faults on the device.  Each failure returns BBGPU_ERR_HIP, leaves no allocation live and staging_bytes where it was, and the next
    call over the same setup is right.  The same over a warm setup: after a failed one no setup exists."""
    import torch
    from barretenberg_amd import BbGpuError
    n, l = 256, 4
    c = coset_polynomials(oracle, n, l)[0][1]
    want = world["twin"](n, l)["random"]
    s = world["setup"](n, l)
    d = dev(c)
    run = lambda: lib.kzg_open_cosets_device(s, d.data_ptr(), n, l)[0]  # noqa: E731
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
            lib.kzg_open_cosets_setup(world["h"], n, l)
        st = lib.fault_stats()
        lib.fault_inject(None)
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"] and st["slots_pending"] == 0, (kind, k, st)
        assert lib.memory_stats()["staging_bytes"] == staging, (kind, k)
    s2 = lib.kzg_open_cosets_setup(world["h"], n, l)
    assert np.array_equal(lib.kzg_open_cosets_device(s2, d.data_ptr(), n, l)[0], want)
    lib.kzg_open_cosets_release(s2)


def test_argument_errors_on_a_bound_device(lib, oracle, world):
    """the verdicts that need a table or a setup; the pool runs out at BBGPU_KZG_OPEN_COSETS_MAX_SETUPS and is not the pool of bbgpu_kzg_open_all_setup:
    both hold the same kind of setup, and this is the guard on their staying two"""
    from barretenberg_amd import BbGpuError
    fake = 0x1000  # never dereferenced
    for n in (2 * ROWS, 1 << 21):  # larger than the table
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_setup(world["h"], n, 64)
    s = world["setup"](256, 4)
    for kw in (dict(stride=255), dict(batch=0), dict(batch=65)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_cosets_device(s, fake, 256, 4, **kw)
    hb = lib.srs_generate(secret_x(oracle), 1 << 16)
    big = lib.kzg_open_cosets_setup(hb, 1 << 16, 64)
    lib.srs_release(hb)  # the setup does not read the table again
    try:
        for batch in (33, 64):  # batch x 2 n above 2^22
            with pytest.raises(BbGpuError, match=ERR_SIZE):
                lib.kzg_open_cosets_device(big, fake, 1 << 16, 64, batch=batch)
        live = lib.fault_stats()["live_allocations"]
        taken, singles = [], []
        with pytest.raises(BbGpuError, match=ERR_STATE):
            for _ in range(17):
                taken.append(lib.kzg_open_cosets_setup(world["h"], 4, 2))
        assert 1 <= len(taken) <= 15 and lib.fault_stats()["live_allocations"] == live + len(taken)
        with pytest.raises(BbGpuError, match=ERR_STATE):  # the other pool: free while this one is full, and filling it frees nothing here
            for _ in range(17):
                singles.append(lib.kzg_open_all_setup(world["h"], 2))
        assert len(singles) == 16
        with pytest.raises(BbGpuError, match=ERR_STATE):
            lib.kzg_open_cosets_setup(world["h"], 4, 2)
        for t in singles:
            lib.kzg_open_all_release(t)
        with pytest.raises(BbGpuError, match=ERR_STATE):
            lib.kzg_open_cosets_setup(world["h"], 4, 2)
        lib.kzg_open_cosets_release(taken.pop())
        taken.append(lib.kzg_open_cosets_setup(world["h"], 4, 2))
        for t in taken:
            lib.kzg_open_cosets_release(t)
        assert lib.fault_stats()["live_allocations"] == live
    finally:
        lib.kzg_open_cosets_release(big)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kzg_open_cosets_release(big)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kzg_open_cosets_device(big, fake, 1 << 16, 64)


def test_a_handle_of_one_pool_is_unknown_to_the_other(lib, oracle, world):
    """both families keep one kind of setup: a number that is live in the pool of bbgpu_kzg_open_all_setup and free in this one is refused by
    bbgpu_kzg_open_cosets_device and bbgpu_kzg_open_cosets_release, and the open-all setup answers as before; then the mirror image with a setup of (4, 2)"""
    from barretenberg_amd import BbGpuError
    n = 4
    cases = polynomials(oracle, n)
    buf = buffer_of(oracle, [c for _, c in cases], n)
    d = dev(buf)
    live = lib.fault_stats()["live_allocations"]
    if len(world["setups"]) == 16:  # no number is free in this pool: give one up
        lib.kzg_open_cosets_release(world["setups"].pop(next(iter(world["setups"]))))
        live -= 1
    singles = [lib.kzg_open_all_setup(world["h"], n)]
    while singles[-1] in world["setups"].values():
        singles.append(lib.kzg_open_all_setup(world["h"], n))
    s = singles[-1]
    try:
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_cosets_device(s, d.data_ptr(), n, 1, batch=len(cases))
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_cosets_release(s)
        want = lib.host_kzg_open_all(aligned_copy(world["table"][:2 * n]), n, buf, batch=len(cases))
        assert np.array_equal(lib.kzg_open_all_device(s, d.data_ptr(), n, batch=len(cases)), want)
    finally:
        for t in singles:
            lib.kzg_open_all_release(t)
    pairs = coset_polynomials(oracle, n, 2)
    d = dev(buffer_of(oracle, [c for _, c in pairs], n))
    want = world["twin"](n, 2)
    s = lib.kzg_open_cosets_setup(world["h"], n, 2)  # the pool of bbgpu_kzg_open_all_setup is empty again: every number is free there
    try:
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_all_device(s, d.data_ptr(), n, batch=len(pairs))
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kzg_open_all_release(s)
        got = lib.kzg_open_cosets_device(s, d.data_ptr(), n, 2, batch=len(pairs))
        for b, (name, _) in enumerate(pairs):
            assert np.array_equal(got[b], want[name]), name
    finally:
        lib.kzg_open_cosets_release(s)
    assert lib.fault_stats()["live_allocations"] == live


def test_kernel_times_are_reported(lib, oracle, world):
    lib.set_timing(1)
    try:
        open_cosets(lib, world["setup"](256, 4), [coset_polynomials(oracle, 256, 4)[0][1]], 256, 4, 256, oracle)
        ms = lib.last_timing()
    finally:
        lib.set_timing(0)
    assert len(ms) == 4 and all(0 < v < 1000 for v in ms), ms  # the sum kernel, the inverse stages, the gather and the forward stages, the finish kernel


def test_shutdown_releases_the_setups(lib, oracle, world):
    """bbgpu_shutdown frees every setup with its rows: the handles are unknown afterwards, and a new start finds the pool empty"""
    from barretenberg_amd import BbGpuError
    s = world["setup"](8, 4)
    extra = lib.kzg_open_cosets_setup(world["h"], 4, 2)
    lib.shutdown()
    try:
        assert lib.fault_stats()["live_allocations"] == 0
        for dead in (s, extra):
            with pytest.raises(BbGpuError, match=ERR_ARG):
                lib.kzg_open_cosets_release(dead)
            with pytest.raises(BbGpuError, match=ERR_ARG):
                lib.kzg_open_cosets_device(dead, 0x1000, 8, 4)
    finally:
        world["reset"]()  # the next call binds the device again
    taken = [lib.kzg_open_cosets_setup(world["h"], 4, 2) for _ in range(16)]
    for t in taken:
        lib.kzg_open_cosets_release(t)
    c = coset_polynomials(oracle, 8, 4)[0][1]
    assert np.array_equal(open_cosets(lib, world["setup"](8, 4), [c], 8, 4, 8, oracle)[0], world["twin"](8, 4)["random"])
