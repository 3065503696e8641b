"""Opening sessions on the GPU (-m gpu): bbgpu_lagrange_opening_begin / _evaluate / _open / _open_folded / _end and bbgpu_fr_fold_device (csrc/poly.hip
bary_inverses: k_bary_denominators with one grid row per point and ONE batch_invert; bary_open_with: k_bary_dot, k_bary_finish, k_bary_quotient over kept
inverses; bary_open_folded: k_bary_fold_dot / k_fold in front of them).  Every comparison is exact.
The results are compared with the host twins -- held to the oracle's definition by tests/test_opening_session_host.py and tests/test_lagrange_open_host.py --
up to 256 values with the oracle directly, and for every point with the EXISTING two device entries called at that z.
Sizes, from the constants the drivers use (PT = 256 threads per workgroup; k_bary_denominators, k_bary_quotient: 4 elements per thread, at most 1024
workgroups; k_bary_dot, k_bary_fold_dot: 8 per thread = 2048 per workgroup, at most 256 workgroups; k_fold: one element per thread; the scans of
batch_invert: 2048 per workgroup): 2, 4, 64 (one wave), 256 (one workgroup), 2048 (one workgroup of the dot kernels), 4096 (two); 2^20 (past both block caps);
4 x 2^21 denominators (4096 scan blocks: the nested scans); 1000 for the fold alone (no power of two, a partial last workgroup)."""
import numpy as np
import pytest

from oracle.pyoracle import FR, PolyOracle, aligned_copy
from tests.lagrange_open_cases import ERR_ARG, ERR_SIZE, PAD, expected_batch, omega, values, z_cases
from tests.opening_session_cases import ERR_STATE, fold, folded_expected, gamma_sets, on_domain, point_sets

pytestmark = pytest.mark.gpu
SMALL = [2, 4, 64, 256, 2048, 4096]
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
# the funnels one warm call at n = 4096 passes.  begin: the session's allocation; launch checks -- k_bary_denominators, the two product scans
# and the scaling of batch_invert.  The session calls: no allocation, no upload, one read-back when values are returned, one launch check for the chain of
# kernels (none for an evaluation on the domain, which is a copy); accumulating adds the launch check of the pass that adds.
def _w(d2h, launch, alloc=0):
    return dict(alloc_calls=alloc, h2d_calls=0, d2h_calls=d2h, launch_checks=launch)


WARM_BEGIN = _w(0, 4, alloc=1)
WARM = {"evaluate": _w(1, 1), "evaluate on": _w(1, 0), "open": _w(1, 1), "open on": _w(1, 1), "open, no f": _w(0, 1), "folded": _w(1, 1), "folded on": _w(1, 1),
        "folded, accumulate": _w(1, 2), "folded on, accumulate, no f": _w(0, 2)}


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


def session_open(lib, s, t, d_v, n, batch, stride, in_place=False, want_f=True):
    import torch
    d_q = d_v.clone() if in_place else torch.full_like(d_v, PAD)
    f = lib.lagrange_opening_open(s, t, d_q.data_ptr() if in_place else d_v.data_ptr(), d_q.data_ptr(), n, batch=batch, stride=stride, want_f=want_f)
    torch.cuda.synchronize()
    return host(d_q), f


def session_folded(lib, s, t, d_v, n, batch, stride, gamma, d_q=None, want_f=True):
    import torch
    acc = d_q is not None
    d_q = torch.full((n + 1, 4), PAD, dtype=torch.int64, device="cuda") if d_q is None else d_q  # one element of guard
    f = lib.lagrange_opening_open_folded(s, t, d_v.data_ptr(), n, gamma, d_q.data_ptr(), batch=batch, stride=stride, accumulate=acc, want_f=want_f)
    torch.cuda.synchronize()
    q = host(d_q)
    assert (q[n] == PAD).all()
    return q[:n], f


@pytest.mark.parametrize("n", SMALL)
def test_sessions_against_twins_oracle_and_the_existing_entries(lib, oracle, n):
    """points 1, 2 and 4, on and off the domain and twice the same; batch 1, 3 with padding, 64 (n = 64 and 4096)"""
    import torch
    shapes = [(1, n), (3, n + 3)] + ([(64, n)] if n in (64, 4096) else [])
    sets = point_sets(oracle, n)
    for batch, stride in shapes:
        v = values(oracle, 0x5E0 + n + batch, n, batch, stride)
        d_v = dev(v)
        gammas = gamma_sets(oracle, batch)
        for k, (sname, points) in enumerate(sets if batch < 64 else sets[2:4]):  # batch 64: four points off the domain, and a mixed set
            s = lib.lagrange_opening_begin(n, np.stack([z for z, _ in points]))
            for t, (z, m) in enumerate(points):
                tag = (batch, sname, t)
                q_want, f_want = lib.host_kate_opening_lagrange(v, z, n=n, batch=batch, stride=stride)
                if n <= 256:
                    f_def, q_def = expected_batch(oracle, v, n, batch, stride, z)
                    assert np.array_equal(f_want, f_def) and np.array_equal(q_want, q_def), tag
                f = lib.lagrange_opening_evaluate(s, t, d_v.data_ptr(), n, batch=batch, stride=stride)
                assert np.array_equal(f, f_want) and np.array_equal(f, lib.evaluate_lagrange_device(d_v.data_ptr(), n, z, batch=batch, stride=stride)), tag
                q, f = session_open(lib, s, t, d_v, n, batch, stride)
                assert np.array_equal(f, f_want) and np.array_equal(q, q_want), tag
                assert (q.reshape(batch, stride, 4)[:, n:] == PAD).all(), tag  # the elements between the polynomials are not written
                d_q = torch.full_like(d_v, PAD)
                f_old = lib.kate_opening_lagrange_device(d_v.data_ptr(), d_q.data_ptr(), n, z, batch=batch, stride=stride)
                torch.cuda.synchronize()
                assert np.array_equal(f, f_old) and np.array_equal(q, host(d_q)), tag
                q, f = session_open(lib, s, t, d_v, n, batch, stride, in_place=True)
                assert np.array_equal(f, f_want) and np.array_equal(q, q_want), tag
                gname, g = gammas[(k + t) % len(gammas)]
                qf_want, ff_want = lib.host_kate_opening_lagrange_folded(v, g, z, n=n, stride=stride)
                if n <= 256:
                    ff_def, qf_def = folded_expected(oracle, v, n, batch, stride, g, z)
                    assert np.array_equal(ff_want, ff_def) and np.array_equal(qf_want, qf_def), (tag, gname)
                qf, ff = session_folded(lib, s, t, d_v, n, batch, stride, g)
                assert np.array_equal(ff, ff_want) and np.array_equal(qf, qf_want), (tag, gname)
            lib.lagrange_opening_end(s)
        assert np.array_equal(host(d_v), v)  # the values are read only


@pytest.mark.parametrize("n", [64, 4096])
def test_accumulate_and_the_fold_alone(lib, oracle, n):
    """accumulate over two calls (different buffers and strides) equals one call over the concatenation and the twin; a caller's stream; no value wanted;
    bbgpu_fr_fold_device against its twin, also at a length that is no power of two"""
    import torch
    va, vb = values(oracle, 0xACC + n, n, 2, n + 3), values(oracle, 0xACD + n, n, 1, n)
    vc = aligned_copy(np.concatenate([va[:n], va[n + 3:2 * n + 3], vb]))
    ga, gb = gamma_sets(oracle, 2)[0][1], gamma_sets(oracle, 1)[3][1]
    gc = aligned_copy(np.concatenate([ga, gb]))
    d_a, d_b, d_c = dev(va), dev(vb), dev(vc)
    cases = z_cases(oracle, n)
    s = lib.lagrange_opening_begin(n, np.stack([cases[0][1], cases[-1][1]]))
    for t, (name, z, _) in enumerate((cases[0], cases[-1])):
        d_q = torch.full((n + 1, 4), PAD, dtype=torch.int64, device="cuda")
        _, fa = session_folded(lib, s, t, d_a, n, 2, n + 3, ga)
        lib.lagrange_opening_open_folded(s, t, d_a.data_ptr(), n, ga, d_q.data_ptr(), stride=n + 3, want_f=False)
        q, fb = session_folded(lib, s, t, d_b, n, 1, n, gb, d_q=d_q)
        q_one, f_one = session_folded(lib, s, t, d_c, n, 3, n, gc)
        q_twin, f_twin = lib.host_kate_opening_lagrange_folded(vc, gc, z, n=n, stride=n)
        assert np.array_equal(q, q_one) and np.array_equal(q, q_twin) and np.array_equal(f_one, f_twin), name
        assert np.array_equal(fa, lib.host_kate_opening_lagrange_folded(va, ga, z, n=n, stride=n + 3)[1]), name  # F(z) is that of each call alone
        assert np.array_equal(fb, lib.host_kate_opening_lagrange_folded(vb, gb, z, n=n, stride=n)[1]), name
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            d_s = torch.full((n, 4), PAD, dtype=torch.int64, device="cuda")
            stream.synchronize()
            f = lib.lagrange_opening_open_folded(s, t, d_c.data_ptr(), n, gc, d_s.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
        assert np.array_equal(f, f_twin) and np.array_equal(host(d_s), q_twin), name
    lib.lagrange_opening_end(s)
    for length, batch, stride in ((n, 2, n + 3), (1000, 3, 1003), (1, 64, 1), (257, 1, 257)):
        v = values(oracle, 0xF0 + length, length, batch, stride) if length > 1 else aligned_copy(oracle.random_scalars(7, batch))
        for gname, g in gamma_sets(oracle, batch)[:5 if length == n else 2]:
            d_out = torch.full((length + 1, 4), PAD, dtype=torch.int64, device="cuda")
            want = lib.host_fold(v, g, n=length, stride=stride)
            lib.fold_device(d_out.data_ptr(), dev(v).data_ptr(), length, g, stride=stride)
            torch.cuda.synchronize()
            assert np.array_equal(host(d_out)[:length], want) and (host(d_out)[length] == PAD).all(), (length, gname)
            lib.fold_device(d_out.data_ptr(), dev(v).data_ptr(), length, g, stride=stride, accumulate=True)
            torch.cuda.synchronize()
            assert np.array_equal(host(d_out)[:length], lib.host_fold(v, g, n=length, stride=stride, out=want.copy())), (length, gname)
            assert (host(d_out)[length] == PAD).all()
        if length <= 1000:
            assert np.array_equal(lib.host_fold(v, g, n=length, stride=stride), fold(v, length, batch, stride, g))


def test_past_the_block_caps(lib, oracle):
    """n = 2^20, two points (off the domain, w^(n/2 + 1)), batch 8 on values drawn on the device: the host twin's fold is uploaded, and open_folded must
    equal the EXISTING bbgpu_kate_opening_lagrange_device on that folded vector, folded_f_of_z its f; bbgpu_fr_fold_device must equal the upload"""
    import torch
    n, batch = 1 << 20, 8
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x0F01D)
    v = torch.randint(-(1 << 63), (1 << 63) - 1, (batch * n, 4), dtype=torch.int64, device="cuda", generator=gen)
    g = gamma_sets(oracle, batch)[4][1]  # random with one representative gamma + r
    d_f = dev(lib.host_fold(host(v), g, n=n, stride=n))
    d_g = torch.empty_like(d_f)
    lib.fold_device(d_g.data_ptr(), v.data_ptr(), n, g)
    torch.cuda.synchronize()
    assert torch.equal(d_g, d_f)
    cases = z_cases(oracle, n)
    zs = [cases[0][1], cases[7][1]]
    assert cases[7][2] == n // 2 + 1
    s = lib.lagrange_opening_begin(n, np.stack(zs))
    d_q, d_ref = torch.empty_like(d_f), torch.empty_like(d_f)
    for t, z in enumerate(zs):
        f = lib.lagrange_opening_open_folded(s, t, v.data_ptr(), n, g, d_q.data_ptr())
        f_ref = lib.kate_opening_lagrange_device(d_f.data_ptr(), d_ref.data_ptr(), n, z)[0]
        torch.cuda.synchronize()
        assert np.array_equal(f, f_ref) and torch.equal(d_q, d_ref), t
    lib.lagrange_opening_end(s)


def test_nested_scans_of_the_inversion(lib, oracle):
    """4 points x 2^21 values = 2^23 denominators in one batch_invert (4096 scan blocks), batch 1, once: evaluate and open at each point against the
    existing entries"""
    import torch
    n = 1 << 21
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x2E57ED)
    v = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=gen)
    off = oracle.random_scalars(0x2E57, 2)
    zs = [off[0], on_domain(n, n // 2 + 1), off[1], on_domain(n, n - 1, lift=True)]
    s = lib.lagrange_opening_begin(n, np.stack(zs))
    d_q, d_ref = torch.empty_like(v), torch.empty_like(v)
    for t, z in enumerate(zs):
        f_ref = lib.kate_opening_lagrange_device(v.data_ptr(), d_ref.data_ptr(), n, z)
        assert np.array_equal(lib.lagrange_opening_evaluate(s, t, v.data_ptr(), n), f_ref), t
        f = lib.lagrange_opening_open(s, t, v.data_ptr(), d_q.data_ptr(), n)
        torch.cuda.synchronize()
        assert np.array_equal(f, f_ref) and torch.equal(d_q, d_ref), t
    lib.lagrange_opening_end(s)


def test_the_proof_verifies(lib, oracle, tmp_path):
    """the PLONK shape at n = 4096 over srs_generate + srs_lagrange: five polynomials, three opened at z and two at z w; commitments over the Lagrange handle,
    evaluations from the session, proof points the MSMs of the two folded quotients.  bbgpu_host_kzg_check_openings accepts, and refuses one y + 1; each
    proof point equals sum_b gamma_b (MSM of the EXISTING entry's quotient b), formed with the oracle's group operations"""
    import torch
    from tests.srs_check_cases import g2_of
    from tests.srs_lagrange_cases import secret_x
    n = 4096
    x = secret_x(oracle)
    g2_x = g2_of(lib, oracle, tmp_path, x, "x.dat")
    h = lib.srs_generate(x, n)
    hl, _, _ = lib.srs_lagrange(h, n)
    try:
        v = values(oracle, 0x9107 + n, n, 5)
        d_v = dev(v)
        torch.cuda.synchronize()  # the MSMs run on streams of their own: what they read must be complete
        at = [d_v.data_ptr() + b * n * 32 for b in range(5)]
        commitments = np.stack([lib.msm_device(hl, at[b], n)[:8] for b in range(5)])
        z = z_cases(oracle, n)[0][1]
        zw = oracle.mul(FR, z, PolyOracle.mont([omega(n)])[0])
        groups = [(z, 0, 3, gamma_sets(oracle, 3)[0][1]), (zw, 3, 2, gamma_sets(oracle, 2)[0][1])]
        s = lib.lagrange_opening_begin(n, np.stack([z, zw]))
        claims = []
        for t, (zt, first, count, g) in enumerate(groups):
            y = lib.lagrange_opening_evaluate(s, t, at[first], n, batch=count)
            d_q = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            yf = lib.lagrange_opening_open_folded(s, t, at[first], n, g, d_q.data_ptr())
            assert np.array_equal(yf, fold(y, 1, count, 1, g)[0]), t  # the folded value is the fold of the values
            torch.cuda.synchronize()
            pi = lib.msm_device(hl, d_q.data_ptr(), n)
            d_each = torch.empty((count * n, 4), dtype=torch.int64, device="cuda")  # the existing entry: one quotient and one MSM per polynomial
            assert np.array_equal(lib.kate_opening_lagrange_device(at[first], d_each.data_ptr(), n, zt, batch=count), y), t
            torch.cuda.synchronize()
            acc = None
            for b in range(count):
                term = oracle.g1_scalar_mul(lib.msm_device(hl, d_each.data_ptr() + b * n * 32, n)[:8], g[b])
                acc = term if acc is None else oracle.g1_add(acc, term)
            assert np.array_equal(oracle.g1_normalize(acc)[:8], pi[:8]), t
            c = lib.host_msm(aligned_copy(g), aligned_copy(commitments[first:first + count]), count, plain=True)[:8]
            claims.append([c, zt, yf, pi[:8]])
        lib.lagrange_opening_end(s)

        def verdict(cl):
            return lib.host_kzg_check_openings(*[np.stack([c[k] for c in cl]) for k in range(4)], g2_x)
        assert verdict(claims)
        for t in range(2):
            bad = [list(c) for c in claims]
            bad[t][2] = oracle.add(FR, bad[t][2], oracle.const(FR, "one"))
            assert not verdict(bad), t
    finally:
        lib.srs_release(hl)
        lib.srs_release(h)
    assert lib.fault_stats()["slots_pending"] == 0


# ---- funnels and memory -------------------------------------------------------------------------------------------------------------------------------
N, BATCH = 4096, 3


def session_points(oracle):
    cases = z_cases(oracle, N)
    return np.stack([cases[0][1], cases[-1][1]])  # point 0 off the domain, point 1 on it


def calls(lib, oracle, s):
    """name -> (a closure that runs one call of session s and returns what it computed, the values it must return)"""
    v = values(oracle, 0xFA18, N, BATCH)
    d_v = dev(v)
    g = gamma_sets(oracle, BATCH)[0][1]
    zs = session_points(oracle)

    def evaluation(t):
        return (lambda: (lib.lagrange_opening_evaluate(s, t, d_v.data_ptr(), N, batch=BATCH),)), (lib.host_evaluate_lagrange(v, zs[t], n=N, batch=BATCH),)

    def opening(t, want_f=True):
        want = lib.host_kate_opening_lagrange(v, zs[t], n=N, batch=BATCH)
        return (lambda: session_open(lib, s, t, d_v, N, BATCH, N, want_f=want_f)[:2 if want_f else 1]), want if want_f else want[:1]

    def folded(t, accumulate=False, want_f=True):
        q, f = lib.host_kate_opening_lagrange_folded(v, g, zs[t], n=N, stride=N)
        if accumulate:
            q = lib.host_kate_opening_lagrange_folded(v, g, zs[t], n=N, stride=N, out=q.copy())[0]

        def run():
            import torch
            d_q = None
            if accumulate:  # onto the quotient itself, made by a call outside what is counted or failed
                d_q = torch.cat([dev(lib.host_kate_opening_lagrange_folded(v, g, zs[t], n=N, stride=N)[0]), torch.full((1, 4), PAD, dtype=torch.int64, device="cuda")])
            return session_folded(lib, s, t, d_v, N, BATCH, N, g, d_q=d_q, want_f=want_f)[:2 if want_f else 1]
        return run, (q, f) if want_f else (q,)
    return {"evaluate": evaluation(0), "evaluate on": evaluation(1), "open": opening(0), "open on": opening(1), "open, no f": opening(0, False),
            "folded": folded(0), "folded on": folded(1), "folded, accumulate": folded(0, True), "folded on, accumulate, no f": folded(1, True, False)}


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_funnel_counts_and_memory(lib, oracle):
    """the warm-call counts DESIGN.md states; a session's inverses are counted in staging_bytes and go with end"""
    zs = session_points(oracle)
    lib.lagrange_opening_end(lib.lagrange_opening_begin(N, zs))  # warm: the temporaries of the inversion are grown
    before, live = lib.memory_stats(), lib.fault_stats()
    s, st = counted(lib, lambda: lib.lagrange_opening_begin(N, zs), WARM_BEGIN)
    print("funnels of one warm begin:", st)
    assert st == WARM_BEGIN
    during = lib.memory_stats()
    assert during["staging_bytes"] == before["staging_bytes"] + 2 * N * 32 and lib.fault_stats()["live_allocations"] == live["live_allocations"] + 1
    assert {k: during[k] for k in during if k != "staging_bytes"} == {k: before[k] for k in before if k != "staging_bytes"}
    for name, (run, want) in calls(lib, oracle, s).items():
        assert same(run(), want), name  # warm
        mem = lib.memory_stats()
        got, st = counted(lib, run, WARM[name])
        print("funnels of one warm call (%s):" % name, st)
        assert same(got, want) and st == WARM[name], (name, st)
        assert lib.memory_stats() == mem, name
    mem = lib.memory_stats()
    lib.lagrange_opening_end(s)
    after = lib.fault_stats()
    assert lib.memory_stats() == dict(mem, staging_bytes=mem["staging_bytes"] - 2 * N * 32)  # the inverses are gone, nothing else
    assert lib.memory_stats() == before and after["live_allocations"] == live["live_allocations"] and after["live_bytes"] == live["live_bytes"]
    s2 = lib.lagrange_opening_begin(N, zs)
    assert lib.fault_stats()["live_allocations"] == after["live_allocations"] + 1
    mem = lib.memory_stats()
    lib.lagrange_opening_end(s2)
    assert lib.fault_stats()["live_allocations"] == after["live_allocations"] and lib.fault_stats()["live_bytes"] == after["live_bytes"]
    assert lib.memory_stats()["staging_bytes"] == mem["staging_bytes"] - 2 * N * 32


def no_session_is_live(lib):
    from barretenberg_amd import BbGpuError
    for k in range(16):
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_end(k)


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures(lib, oracle, kind):
    """every site of the funnel `kind` that a warm call passes, failed once.  These are host-side funnels; nothing faults on the device.  After a failed
    begin no session exists and the live allocations are those of before; after a failed session call the same call succeeds and returns the right words"""
    from barretenberg_amd import BbGpuError
    zs = session_points(oracle)
    lib.lagrange_opening_end(lib.lagrange_opening_begin(N, zs))  # warm
    no_session_is_live(lib)
    before = lib.fault_stats()
    for k in range(WARM_BEGIN[KEYS[kind]]):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError):
            lib.lagrange_opening_begin(N, zs)
        st = lib.fault_stats()
        lib.fault_inject(None)
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"] and st["slots_pending"] == 0, (kind, k, st)
        no_session_is_live(lib)
    s = lib.lagrange_opening_begin(N, zs)
    before = lib.fault_stats()
    for name, (run, want) in calls(lib, oracle, s).items():
        assert same(run(), want), name  # warm
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
            assert same(run(), want), (name, kind, k)  # the session stays usable
    lib.lagrange_opening_end(s)
    assert lib.fault_stats()["live_allocations"] == before["live_allocations"] - 1


def test_sessions_run_out_and_argument_errors_on_a_bound_device(lib, oracle):
    from barretenberg_amd import BbGpuError
    n = 64
    z = oracle.random_scalars(3, 4)
    d_v = dev(values(oracle, 5, n, 2))
    p, g = d_v.data_ptr(), gamma_sets(oracle, 2)[0][1]
    live = lib.fault_stats()["live_allocations"]
    sessions = [lib.lagrange_opening_begin(n, z[:1 + k % 4]) for k in range(16)]
    assert sorted(sessions) == list(range(16))
    with pytest.raises(BbGpuError, match=ERR_STATE):
        lib.lagrange_opening_begin(n, z[:1])  # the 17th
    assert lib.fault_stats()["live_allocations"] == live + 16
    for s in sessions[1:]:
        lib.lagrange_opening_end(s)
    s = sessions[0]  # one point
    assert lib.fault_stats()["live_allocations"] == live + 1
    for kw in (dict(n=0), dict(n=1), dict(n=48), dict(n=1 << 25), dict(n=n, points=0), dict(n=n, points=5), dict(n=1 << 23, points=4)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_begin(z=z, **kw)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.lagrange_opening_begin(n, None, points=1)
    for kw in (dict(batch=0), dict(batch=65), dict(batch=2, stride=n - 1)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_evaluate(s, 0, p, n, **kw)
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_open(s, 0, p, p, n, **kw)
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_open_folded(s, 0, p, n, g, p, **kw)
    for session, point in ((s, 1), (s, -1), (1, 0), (16, 0), (-1, 0)):  # a point outside the session, ended and unknown sessions
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_evaluate(session, point, p, n)
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_open(session, point, p, p, n)
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_open_folded(session, point, p, n, g, p)
    for call in (lambda: lib.lagrange_opening_evaluate(s, 0, None, n), lambda: lib.lagrange_opening_open(s, 0, None, p, n),
                 lambda: lib.lagrange_opening_open(s, 0, p, None, n), lambda: lib.lagrange_opening_open_folded(s, 0, None, n, g, p),
                 lambda: lib.lagrange_opening_open_folded(s, 0, p, n, g, None), lambda: lib.lagrange_opening_open_folded(s, 0, p, n, None, p, batch=2),
                 lambda: lib.fold_device(None, p, n, g), lambda: lib.fold_device(p, None, n, g), lambda: lib.fold_device(p, p, n, None, batch=2)):
        with pytest.raises(BbGpuError, match=ERR_ARG):
            call()
    for kw in (dict(n=0), dict(n=(1 << 24) + 1), dict(n=n, batch=0), dict(n=n, batch=65), dict(n=n, stride=n - 1)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.fold_device(p, p, gamma=g, **kw)
    assert np.array_equal(lib.lagrange_opening_evaluate(s, 0, p, n, batch=2), lib.host_evaluate_lagrange(host(d_v), z[0], n=n, batch=2))  # still usable
    lib.lagrange_opening_end(s)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.lagrange_opening_end(s)
    assert lib.fault_stats()["live_allocations"] == live
