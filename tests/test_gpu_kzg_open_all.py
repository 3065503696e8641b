"""bbgpu_kzg_open_all_setup / bbgpu_kzg_open_all_device on the GPU (-m gpu): the kernels of csrc/kzg_open_cosets.hip at coset size 1 (the string and
its transform, the scalars of t, the sum kernel that at this size multiplies each row by its own scalar and adds nothing, both group transforms over a
batch, the gather, the normalisation with infinities) against the host twin bit for bit -- itself held to the quotient definition by tests/test_kzg_open_all_host.py -- against the device's own per-point path, and against
the pairing check.  Sizes: n = 2, 4 (the shortest transforms), 32 (N = 64: one workgroup), 64 (N = 128: the first size at which k_lagrange_stage takes its
groups-per-wave addressing), 256 with batch 1, 3 and 16 (both addressings in several stages, and the batch dimension), 4096 through the pairing check."""
import numpy as np
import pytest

from oracle.pyoracle import FR, aligned_copy
from tests.kzg_open_all_cases import ERR_ARG, ERR_SIZE, ERR_STATE, INF, PAD, buffer_of, domain, infinite_row_table, polynomials, secret_x

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
ROWS = 4096
# the funnels one warm call at n = 64 passes (include/bbgpu.h): allocations -- t (later the proofs) and the scratch points; no upload; read-backs -- the
# proofs (one staging chunk); launch checks -- k_open_cosets_t, the transform of t, the chain from the sum kernel to the finish kernel
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
    """the generated table of a known x (handle and host copy), one setup per size, and per size the host twin's proofs of every polynomial of the cases
    module (one twin call per size): made once, never written to"""
    h, table = lib.srs_generate(secret_x(oracle), ROWS, want_host_table=True)
    setups, twins = {}, {}

    def setup(n):
        if n not in setups:
            setups[n] = lib.kzg_open_all_setup(h, n)
        return setups[n]

    def twin(n):
        if n not in twins:
            cases = polynomials(oracle, n)
            got = lib.host_kzg_open_all(aligned_copy(table[:2 * n]), n, buffer_of(oracle, [c for _, c in cases], n), batch=len(cases))
            twins[n] = {name: got[k] for k, (name, _) in enumerate(cases)}
        return twins[n]
    yield dict(h=h, table=table, setup=setup, twin=twin)
    for s in setups.values():
        lib.kzg_open_all_release(s)


def open_all(lib, setup, polys, n, stride, oracle):
    """one device call over the polynomials `polys`; the input on the device is unchanged afterwards"""
    import torch
    buf = buffer_of(oracle, polys, stride)
    d = dev(buf)
    got = lib.kzg_open_all_device(setup, d.data_ptr(), n, batch=len(polys), stride=stride)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy().view(np.uint64), buf)
    return got


@pytest.mark.parametrize("n,batch,pad", [(2, 1, 0), (2, 3, PAD), (4, 1, 0), (4, 3, PAD), (32, 1, 0), (32, 3, PAD), (64, 1, 0), (64, 3, PAD), (256, 1, 0),
                                         (256, 3, PAD), (256, 16, 0)])
def test_device_against_twin(lib, oracle, world, n, batch, pad):
    """every polynomial of the cases module, `batch` of them per call (the list wraps), bit for bit"""
    cases, want = polynomials(oracle, n), world["twin"](n)
    for k in range(0, len(cases), batch):
        group = [cases[(k + b) % len(cases)] for b in range(batch)]
        got = open_all(lib, world["setup"](n), [c for _, c in group], n, n + pad, oracle)
        for b, (name, _) in enumerate(group):
            assert np.array_equal(got[b], want[name]), (name, b)
    assert np.array_equal(want["constant"], np.tile(INF, (n, 1))) and np.array_equal(want["X"], np.tile(world["table"][0], (n, 1)))
    assert lib.fault_stats()["slots_pending"] == 0


def test_device_against_its_own_per_point_path(lib, oracle, world):
    """n = 64: bbgpu_kate_opening_device at omega^i, then bbgpu_msm_g1_device over the same handle, for all 64 points"""
    import torch
    n = 64
    c = polynomials(oracle, n)[0][1]
    got = open_all(lib, world["setup"](n), [c], n, n, oracle)[0]
    d_c, d_q = dev(c), torch.empty((n, 4), dtype=torch.int64, device="cuda")
    for i, z in enumerate(domain(oracle, n)):
        lib.compute_kate_opening_coefficients_device(d_c.data_ptr(), d_q.data_ptr(), n, z)
        torch.cuda.synchronize()  # the MSM runs on a stream of its own: what it reads must be complete
        assert np.array_equal(got[i], lib.msm_device(world["h"], d_q.data_ptr(), n)[:8]), i


def test_sampled_proofs_pass_the_pairing_check(lib, oracle, world, tmp_path):
    """n = 4096, batch 2: 64 proofs at fixed indices, with y_i from bbgpu_ntt_device and the commitments from the device MSM, are accepted by
    bbgpu_host_kzg_check_openings; one altered y is rejected"""
    import torch
    from tests.srs_check_cases import SEED, g2_of
    n, batch = 4096, 2
    g2_x = g2_of(lib, oracle, tmp_path, secret_x(oracle), "x.dat")
    c = aligned_copy(oracle.random_scalars(0x4096, batch * n))
    d_c = dev(c)
    setup = lib.kzg_open_all_setup(world["h"], n)
    try:
        proofs = lib.kzg_open_all_device(setup, d_c.data_ptr(), n, batch=batch)
    finally:
        lib.kzg_open_all_release(setup)
    d_y = d_c.clone()
    torch.cuda.synchronize()
    commitments = [lib.msm_device(world["h"], d_c.data_ptr() + b * n * 32, n)[:8] for b in range(batch)]
    lib.ntt_device_batch(d_y.data_ptr(), n, batch, "fft")
    torch.cuda.synchronize()
    y = d_y.cpu().numpy().view(np.uint64).reshape(batch, n, 4)
    zs = domain(oracle, n)
    picks = [(k % batch, (k * 2731 + 17 * (k % 3)) % n) for k in range(60)] + [(0, 0), (1, n - 1), (0, n // 2), (1, 1)]
    claims = [np.stack([commitments[b] for b, _ in picks]), np.stack([zs[i] for _, i in picks]), np.stack([y[b, i] for b, i in picks]),
              np.stack([proofs[b, i] for b, i in picks])]
    assert lib.host_kzg_check_openings(*claims, g2_x, seed=SEED)
    claims[2] = claims[2].copy()
    claims[2][37] = oracle.add(FR, claims[2][37], oracle.const(FR, "one"))
    assert not lib.host_kzg_check_openings(*claims, g2_x, seed=SEED)


def test_a_string_whose_transform_has_a_row_at_infinity(lib, oracle):
    """x = W zeta at n = 4: row 1 of S^ is the point at infinity; the setup keeps it and the proofs are the twin's"""
    table = infinite_row_table(oracle)
    h = lib.srs_register(table)
    try:
        setup = lib.kzg_open_all_setup(h, 4)
        try:
            cases = polynomials(oracle, 4)
            want = lib.host_kzg_open_all(table, 4, buffer_of(oracle, [c for _, c in cases], 4), batch=len(cases))
            assert np.array_equal(open_all(lib, setup, [c for _, c in cases], 4, 4, oracle), want)
        finally:
            lib.kzg_open_all_release(setup)
    finally:
        lib.srs_release(h)


def test_a_row_off_the_curve_is_named_and_no_setup_is_made(lib, oracle, world):
    from barretenberg_amd import BbGpuError
    from tests.srs_update_cases import tampered
    n = 64
    h = lib.srs_register(tampered(world["table"][:2 * n], 37))
    try:
        live = lib.fault_stats()["live_allocations"]
        with pytest.raises(BbGpuError, match=ERR_ARG + ".*row 37 "):
            lib.kzg_open_all_setup(h, n)
        assert lib.fault_stats()["live_allocations"] == live
    finally:
        lib.srs_release(h)
    h = lib.srs_register(tampered(world["table"][:2 * n], n - 1))  # row n - 1 is not read
    try:
        lib.kzg_open_all_release(lib.kzg_open_all_setup(h, n))
    finally:
        lib.srs_release(h)


def test_setup_memory_is_counted_and_returned(lib, oracle, world):
    """setup, call, release and setup again leave bbgpu_memory_stats where it was; the rows of S^ are counted in staging_bytes while the setup lives"""
    n = 64
    c = polynomials(oracle, n)[0][1]
    s = lib.kzg_open_all_setup(world["h"], n)  # warm: the staging of the curve findings and of the transform is grown
    open_all(lib, s, [c], n, n, oracle)
    lib.kzg_open_all_release(s)
    before, live = lib.memory_stats(), lib.fault_stats()
    for _ in range(2):
        s = lib.kzg_open_all_setup(world["h"], n)
        during = lib.memory_stats()
        assert during == dict(before, staging_bytes=before["staging_bytes"] + 2 * n * 128)
        assert lib.fault_stats()["live_allocations"] == live["live_allocations"] + 1
        assert np.array_equal(open_all(lib, s, [c], n, n, oracle)[0], world["twin"](n)["random"])
        assert lib.memory_stats() == during
        lib.kzg_open_all_release(s)
        after = lib.fault_stats()
        assert lib.memory_stats() == before and after["live_allocations"] == live["live_allocations"] and after["live_bytes"] == live["live_bytes"]


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_funnel_counts_of_warm_calls(lib, oracle, world):
    n = 64
    c = polynomials(oracle, n)[0][1]
    lib.kzg_open_all_release(lib.kzg_open_all_setup(world["h"], n))  # warm
    s, st = counted(lib, lambda: lib.kzg_open_all_setup(world["h"], n), WARM_SETUP)
    lib.kzg_open_all_release(s)
    print("funnels of one warm setup at n = 64:", st)
    assert st == WARM_SETUP
    run = lambda: open_all(lib, world["setup"](n), [c], n, n, oracle)[0]  # noqa: E731
    run()
    got, st = counted(lib, run, WARM)
    print("funnels of one warm call at n = 64:", st)
    assert np.array_equal(got, world["twin"](n)["random"]) and st == WARM


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, oracle, world, kind):
    """every site of the funnel `kind` that one warm call at n = 64 passes, failed once.  These are host-side funnels (the library's failure injection of
    API results); nothing faults on the device.  Each failure returns BBGPU_ERR_HIP, leaves no allocation live, and the next call over the same setup is
    right.  The same over a warm setup: after a failed one no setup exists."""
    import torch
    from barretenberg_amd import BbGpuError
    n = 64
    c = polynomials(oracle, n)[0][1]
    want = world["twin"](n)["random"]
    s = world["setup"](n)
    d = dev(c)
    run = lambda: lib.kzg_open_all_device(s, d.data_ptr(), n)[0]  # noqa: E731
    assert np.array_equal(run(), want)  # warm
    before = lib.fault_stats()
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
        assert np.array_equal(run(), want), (kind, k)  # the setup stays usable
    for k in range(WARM_SETUP[KEYS[kind]]):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError, match=" -1:"):
            lib.kzg_open_all_setup(world["h"], n)
        st = lib.fault_stats()
        lib.fault_inject(None)
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"] and st["slots_pending"] == 0, (kind, k, st)
    s2 = lib.kzg_open_all_setup(world["h"], n)
    assert np.array_equal(lib.kzg_open_all_device(s2, d.data_ptr(), n)[0], want)
    lib.kzg_open_all_release(s2)


def test_argument_errors_on_a_bound_device(lib, oracle, world):
    """the verdicts that need a table or a setup; setups run out at BBGPU_KZG_OPEN_ALL_MAX_SETUPS"""
    from barretenberg_amd import BbGpuError
    fake = 0x1000  # never dereferenced
    for n in (2 * ROWS, 1 << 21):  # larger than the table
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_all_setup(world["h"], n)
    s = world["setup"](64)
    for kw in (dict(stride=63), dict(batch=0), dict(batch=65)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.kzg_open_all_device(s, fake, 64, **kw)
    hb = lib.srs_generate(secret_x(oracle), 1 << 16)
    big = lib.kzg_open_all_setup(hb, 1 << 16)
    lib.srs_release(hb)  # the setup does not read the table again
    try:
        for batch in (33, 64):  # batch x 2 n above 2^22
            with pytest.raises(BbGpuError, match=ERR_SIZE):
                lib.kzg_open_all_device(big, fake, 1 << 16, batch=batch)
        live = lib.fault_stats()["live_allocations"]
        taken = []
        with pytest.raises(BbGpuError, match=ERR_STATE):
            for _ in range(17):
                taken.append(lib.kzg_open_all_setup(world["h"], 2))
        assert 1 <= len(taken) <= 15 and lib.fault_stats()["live_allocations"] == live + len(taken)
        for t in taken:
            lib.kzg_open_all_release(t)
        assert lib.fault_stats()["live_allocations"] == live
    finally:
        lib.kzg_open_all_release(big)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kzg_open_all_release(big)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.kzg_open_all_device(big, fake, 1 << 16)


def test_kernel_times_are_reported(lib, oracle, world):
    lib.set_timing(1)
    try:
        open_all(lib, world["setup"](256), [polynomials(oracle, 256)[0][1]], 256, 256, oracle)
        ms = lib.last_timing()
    finally:
        lib.set_timing(0)
    assert len(ms) == 4 and all(0 < v < 1000 for v in ms), ms  # the sum kernel (no tree at l = 1), the inverse stages, the gather and the forward stages, the finish kernel
