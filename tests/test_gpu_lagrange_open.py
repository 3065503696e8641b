"""bbgpu_fr_evaluate_lagrange_device / bbgpu_kate_opening_lagrange_device on the GPU (-m gpu): evaluation and opening of polynomials given by their values
on the domain (csrc/poly.hip bary_open: k_bary_denominators, batch_invert, k_bary_dot, k_bary_finish, k_bary_quotient).  Every comparison is exact.
Up to 4096 values the results are compared with the host twins -- themselves held to the definition by tests/test_lagrange_open_host.py -- and, up to 256,
with the oracle's values directly; from 2^16 on with the library's own coefficient-form path (bbgpu_ntt_device + bbgpu_fr_evaluate_device /
bbgpu_kate_opening_device + fft) on inputs drawn on the device.
Sizes, from the constants the drivers use (PT = 256 threads per workgroup; k_bary_denominators and k_bary_quotient: strided_blocks, 4 elements per thread,
at most 1024 workgroups; k_bary_dot: eval_blocks, 8 elements per thread = 2048 per workgroup, at most 256 workgroups; the scans of batch_invert: SCAN_BLOCK =
2048 elements per workgroup, one level up to 2048 blocks): 2 (the smallest domain), 4, 64 (one wave), 256 (one workgroup), 2048 (one workgroup of the dot
kernel at 8 per thread), 4096 (two), 2^16, 2^20 (past both block caps: threads stride more than once), 2^23 (4096 scan blocks: batch_invert's nested
scans; once, batch 1).  z on the domain at m = 0, 1, 63, 64, n/2, n - 1 puts element m in a first lane, a last lane of a wave and a partial block."""
import numpy as np
import pytest

from tests.lagrange_open_cases import ERR_ARG, ERR_SIZE, PAD, expected_batch, values, z_cases

pytestmark = pytest.mark.gpu
SMALL = [2, 4, 64, 256, 2048, 4096]
EXTRA_M = (0, 1, 63, 64)
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
# the funnels one warm call at n = 4096 passes: no allocation and no upload; one read-back, of the values f_b(z), when they are wanted;
# launch checks -- k_bary_denominators, the two product scans and the scaling of batch_invert, and the chain of dot, finish and quotient kernels.
# Evaluation at z on the domain is a copy and a read-back.
WARM = {"evaluate": dict(alloc_calls=0, h2d_calls=0, d2h_calls=1, launch_checks=5), "evaluate on": dict(alloc_calls=0, h2d_calls=0, d2h_calls=1, launch_checks=0),
        "open": dict(alloc_calls=0, h2d_calls=0, d2h_calls=1, launch_checks=5), "open on": dict(alloc_calls=0, h2d_calls=0, d2h_calls=1, launch_checks=5),
        "open, no f": dict(alloc_calls=0, h2d_calls=0, d2h_calls=0, launch_checks=5)}


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
    return t.cpu().numpy().view(np.uint64)


def open_on_device(lib, v, z, n, batch, stride, in_place=False, want_f=True, stream=None):
    import torch
    d_v = dev(v)
    d_q = d_v if in_place else torch.full_like(d_v, PAD)
    f = lib.kate_opening_lagrange_device(d_v.data_ptr(), d_q.data_ptr(), n, z, batch=batch, stride=stride, want_f=want_f, stream=stream)
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(host(d_v), v)  # the values are read only
    return host(d_q), f


def test_memory_grows_by_scratch_only(lib, oracle):
    """the first call of the module's library (nothing is warm): bbgpu_memory_stats differs in the scratch -- staging_bytes -- and its pinned page alone"""
    n = 1 << 12
    d_v = dev(values(oracle, 0x3E3, n))
    before = lib.memory_stats()
    lib.evaluate_lagrange_device(d_v.data_ptr(), n, z_cases(oracle, n)[0][1])
    after = lib.memory_stats()
    assert after["staging_bytes"] > before["staging_bytes"]
    rest = [k for k in after if k not in ("staging_bytes", "pinned_host_bytes")]
    assert {k: after[k] for k in rest} == {k: before[k] for k in rest}


@pytest.mark.parametrize("n", SMALL)
def test_host_parity(lib, oracle, n):
    """batch 3 with padding: evaluation, opening, opening in place, at every kind of z; the oracle's values directly up to 256"""
    batch, stride = 3, n + 3
    v = values(oracle, 0x6B0 + n, n, batch, stride)
    d_v = dev(v)
    for name, z, m in z_cases(oracle, n, EXTRA_M):
        q_want, f_want = lib.host_kate_opening_lagrange(v, z, n=n, batch=batch, stride=stride)
        if n <= 256:
            f_def, q_def = expected_batch(oracle, v, n, batch, stride, z)
            assert np.array_equal(f_want, f_def) and np.array_equal(q_want, q_def), name
        assert np.array_equal(lib.evaluate_lagrange_device(d_v.data_ptr(), n, z, batch=batch, stride=stride), f_want), name
        q, f = open_on_device(lib, v, z, n, batch, stride)
        assert np.array_equal(f, f_want) and np.array_equal(q, q_want), name
        assert (q.reshape(batch, stride, 4)[:, n:] == PAD).all(), name  # the elements between the polynomials are not written
        q, f = open_on_device(lib, v, z, n, batch, stride, in_place=True)
        assert np.array_equal(f, f_want) and np.array_equal(q, q_want), name
    assert np.array_equal(host(d_v), v)


@pytest.mark.parametrize("n", [64, 4096])
def test_batches_streams_and_no_value(lib, oracle, n):
    """batch 1 and 64 at stride n; f_of_z == NULL; a caller's stream"""
    import torch
    stream = torch.cuda.Stream()
    for batch in (1, 64):
        v = values(oracle, 0xBA7 + n + batch, n, batch)
        for name, z, m in z_cases(oracle, n)[:1] + z_cases(oracle, n)[-1:]:  # one off the domain, one on it
            q_want, f_want = lib.host_kate_opening_lagrange(v, z, n=n, batch=batch)
            q, f = open_on_device(lib, v, z, n, batch, n, want_f=False)
            assert f is None and np.array_equal(q, q_want), (batch, name)
            with torch.cuda.stream(stream):
                d_v = dev(v)
                stream.synchronize()
                got = lib.evaluate_lagrange_device(d_v.data_ptr(), n, z, batch=batch, stream=stream.cuda_stream)
                q, f = open_on_device(lib, v, z, n, batch, n, in_place=True, stream=stream.cuda_stream)
            assert np.array_equal(got, f_want) and np.array_equal(f, f_want) and np.array_equal(q, q_want), (batch, name)


@pytest.fixture(scope="module")
def drawn():
    """per (n, batch): values drawn on the device (every 256-bit pattern) and their coefficients by the library's inverse transform; made once"""
    import torch
    cache = {}

    def get(lib, n, batch):
        if (n, batch) not in cache:
            g = torch.Generator(device="cuda")
            g.manual_seed(0x1A6 + n + batch)
            v = torch.randint(-(1 << 63), (1 << 63) - 1, (batch * n, 4), dtype=torch.int64, device="cuda", generator=g)
            c = v.clone()
            lib.ntt_device_batch(c.data_ptr(), n, batch, "ifft")
            torch.cuda.synchronize()
            cache.clear()  # one set at a time: 2^23 elements are 256 MiB a vector
            cache[(n, batch)] = (v, c)
        return cache[(n, batch)]
    return get


@pytest.mark.parametrize("n,batch", [(1 << 16, 1), (1 << 16, 3), (1 << 20, 1), (1 << 20, 3), (1 << 23, 1)])
def test_against_the_coefficient_form(lib, oracle, drawn, n, batch):
    """out[b] == bbgpu_fr_evaluate_device(ifft(values_b), z) and the quotient == fft(bbgpu_kate_opening_device(ifft(values_b), z)), bit for bit"""
    import torch
    v, c = drawn(lib, n, batch)
    cases = z_cases(oracle, n, EXTRA_M)
    if n == 1 << 23:
        cases = [cases[0], cases[7]]  # once off the domain, once on it (w^(n/2 + 1))
    q_ref, q = torch.empty_like(v), torch.empty_like(v)
    for name, z, m in cases:
        f_ref = np.zeros((batch, 4), dtype=np.uint64)
        for b in range(batch):
            f_ref[b] = lib.compute_kate_opening_coefficients_device(c[b * n:].data_ptr(), q_ref[b * n:].data_ptr(), n, z)
            assert np.array_equal(f_ref[b], lib.evaluate_device(c[b * n:].data_ptr(), n, z)), name
        lib.ntt_device_batch(q_ref.data_ptr(), n, batch, "fft")
        assert np.array_equal(lib.evaluate_lagrange_device(v.data_ptr(), n, z, batch=batch), f_ref), name
        f = lib.kate_opening_lagrange_device(v.data_ptr(), q.data_ptr(), n, z, batch=batch)
        torch.cuda.synchronize()
        assert np.array_equal(f, f_ref) and torch.equal(q, q_ref), name
    w = v.clone()  # in place, at the last z (on the domain)
    lib.kate_opening_lagrange_device(w.data_ptr(), w.data_ptr(), n, z, batch=batch, want_f=False)
    torch.cuda.synchronize()
    assert torch.equal(w, q_ref)


@pytest.mark.parametrize("n", [4096, 1 << 14])
def test_the_opening_proof_verifies(lib, oracle, tmp_path, n):
    """the reason the entries exist: with C = sum_i v_i L_i, y = f(z) and pi = sum_i q_i L_i (all over the Lagrange handle),
    e(C - y G + z pi, G2) e(-pi, x G2) == 1, and not for y + 1; pi equals the commitment of the coefficient-form quotient over the monomial handle"""
    import torch
    from oracle.pyoracle import FQ, FR
    from tests.srs_check_cases import g2_of
    from tests.srs_lagrange_cases import secret_x
    x = secret_x(oracle)
    g2_x, g2 = g2_of(lib, oracle, tmp_path, x, "x.dat"), g2_of(lib, oracle, tmp_path, oracle.const(FR, "one"), "one.dat")
    h = lib.srs_generate(x, n)
    hl, _, _ = lib.srs_lagrange(h, n)
    try:
        v = values(oracle, 0xE2E + n, n)
        d_v = dev(v)
        d_c = d_v.clone()
        lib.ntt_device(d_c.data_ptr(), n, "ifft")
        torch.cuda.synchronize()  # the MSMs run on streams of their own: what they read must be complete
        commitment = lib.msm_device(hl, d_v.data_ptr(), n)
        assert np.array_equal(commitment, lib.msm_device(h, d_c.data_ptr(), n))
        G = oracle.g1_one_affine()

        def neg(p12):
            p = np.array(p12, dtype=np.uint64)
            p[4:8] = oracle.neg(FQ, p[4:8])
            return p
        for name, z, m in (z_cases(oracle, n)[0], z_cases(oracle, n)[-1]):  # off the domain, on it
            d_q, d_qc = torch.empty_like(d_v), torch.empty_like(d_v)
            y = lib.kate_opening_lagrange_device(d_v.data_ptr(), d_q.data_ptr(), n, z)[0]
            pi = lib.msm_device(hl, d_q.data_ptr(), n)
            assert np.array_equal(lib.compute_kate_opening_coefficients_device(d_c.data_ptr(), d_qc.data_ptr(), n, z), y), name
            torch.cuda.synchronize()  # that entry returns f(z) before its quotient is complete
            assert np.array_equal(pi, lib.msm_device(h, d_qc.data_ptr(), n)), name
            z_pi = oracle.g1_scalar_mul(pi[:8], z)
            for y_claimed, verdict in ((y, True), (oracle.add(FR, y, oracle.const(FR, "one")), False)):
                lhs = oracle.g1_add(oracle.g1_add(commitment, neg(oracle.g1_scalar_mul(G, y_claimed))), z_pi)
                ps = np.stack([oracle.g1_normalize(lhs)[:8], neg(pi)[:8]])
                assert lib.host_pairing_check(ps, np.stack([g2, g2_x])) == verdict, (name, verdict)
    finally:
        lib.srs_release(hl)
        lib.srs_release(h)
    assert lib.fault_stats()["slots_pending"] == 0


def calls(lib, oracle, n=4096, batch=3):
    """name -> a closure that runs one call at n = 4096 and returns what it computed, and the value it must return"""
    v = values(oracle, 0xFA17, n, batch)
    d_v = dev(v)
    off, on = z_cases(oracle, n)[0][1], z_cases(oracle, n)[-1][1]

    def opening(z, want_f=True):
        def run():
            q, f = open_on_device(lib, v, z, n, batch, n, want_f=want_f)
            return (q, f) if want_f else (q,)
        want = lib.host_kate_opening_lagrange(v, z, n=n, batch=batch)
        return run, want if want_f else want[:1]

    def evaluation(z):
        return (lambda: (lib.evaluate_lagrange_device(d_v.data_ptr(), n, z, batch=batch),)), (lib.host_evaluate_lagrange(v, z, n=n, batch=batch),)
    return {"evaluate": evaluation(off), "evaluate on": evaluation(on), "open": opening(off), "open on": opening(on), "open, no f": opening(off, False)}


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_funnel_counts_and_memory_of_a_warm_call(lib, oracle):
    for name, (run, want) in calls(lib, oracle).items():
        assert same(run(), want), name  # warm
        before = lib.memory_stats()
        lib.fault_inject("launch:%d" % FAR)
        assert same(run(), want), name
        st = lib.fault_stats()
        lib.fault_inject(None)
        print("funnels of one warm call (%s):" % name, {k: st[k] for k in WARM[name]})
        assert {k: st[k] for k in WARM[name]} == WARM[name], (name, st)
        assert lib.memory_stats() == before, name  # no table kept, nothing grown by a second call


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, oracle, kind):
    """every site of the funnel `kind` that a warm call passes, failed once.  These are host-side funnels; nothing faults on the device.  The call returns
    an error, the live allocations and bytes are those of before, no MSM slot is pending, and the next call is right."""
    from barretenberg_amd import BbGpuError
    for name, (run, want) in calls(lib, oracle).items():
        assert same(run(), want), name  # warm
        before = lib.fault_stats()
        for k in range(WARM[name][KEYS[kind]] + 1):  # k == sites: the armed failure no longer fires
            lib.fault_inject("%s:%d" % (kind, k))
            if k < WARM[name][KEYS[kind]]:
                with pytest.raises(BbGpuError):
                    run()
                st = lib.fault_stats()
                assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (name, kind, k, st)
            else:
                assert same(run(), want), (name, kind, k)
                st = lib.fault_stats()
                assert st["fired"] == 0 and st["armed"] == 1, (name, kind, k, st)
            lib.fault_inject(None)
            st = lib.fault_stats()
            assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (name, kind, k, st)
            assert same(run(), want), (name, kind, k)


def test_argument_errors_on_a_bound_device(lib, oracle):
    from barretenberg_amd import BbGpuError
    n = 64
    d_v = dev(values(oracle, 5, n, 2))
    z = z_cases(oracle, n)[0][1]
    p = d_v.data_ptr()
    live = lib.fault_stats()["live_allocations"]
    for kw, code in ((dict(n=0), ERR_SIZE), (dict(n=1), ERR_SIZE), (dict(n=48), ERR_SIZE), (dict(n=1 << 25), ERR_SIZE), (dict(n=n, batch=0), ERR_SIZE),
                     (dict(n=n, batch=65), ERR_SIZE), (dict(n=n, batch=2, stride=n - 1), ERR_SIZE)):
        with pytest.raises(BbGpuError, match=code):
            lib.evaluate_lagrange_device(p, z=z, **kw)
        with pytest.raises(BbGpuError, match=code):
            lib.kate_opening_lagrange_device(p, p, z=z, **kw)
    for args in ((None, p), (p, None)):
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.kate_opening_lagrange_device(args[0], args[1], n, z)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.evaluate_lagrange_device(None, n, z)
    assert lib.fault_stats()["live_allocations"] == live
