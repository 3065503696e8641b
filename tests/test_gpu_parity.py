"""GPU parity tests (-m gpu): libbbgpu.so through its C ABI vs the oracle and the reference-generated fixtures.
Bit-exact bar: integer work, no tolerance."""
import numpy as np
import pytest

from oracle.pyoracle import FQ, FR, FR_MODULUS, NTT_KINDS, aligned_copy
from tests.util import CONST_SEED, NTT_SEED, SCALAR_SEED, SRS_SEED, limbs, noncanonical, sha

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["window-tables", "no-tables"])
def gpu(request):
    """every test runs twice: with the pre-shifted SRS window tables (default) and without (bbgpu_set_precompute(0))"""
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    g.set_host_thresholds(0, 0)  # every size on the GPU kernels (the host answers to tiny sizes are tested in tests/test_host_small.py)
    g.set_precompute(request.param == "window-tables")
    yield g
    g.shutdown()


@pytest.fixture(scope="module")
def const(oracle):
    return oracle.random_scalars(CONST_SEED, 1)[0]


# ------------------------------------------------------------------ NTT ----------------------------------------------
@pytest.mark.parametrize("log2n", [1, 2, 3, 4, 5, 8, 10, 11, 12, 13])
def test_ntt_vs_oracle_all_kinds(gpu, oracle, const, log2n):
    n = 1 << log2n
    co = noncanonical(oracle.random_scalars(NTT_SEED + log2n, n), FR_MODULUS)
    for kind in NTT_KINDS:
        want = oracle.ntt(co, kind, const)
        got = gpu.ntt(co.copy(), kind, const)
        assert np.array_equal(got, want), (log2n, kind)


@pytest.mark.parametrize("log2n", [3, 10, 12, 14])
def test_ntt_batched_launch_equals_single(gpu, oracle, const, log2n):
    """bbgpu_ntt_device_batch: several transforms per launch (single-pass and two-pass sizes, padded stride) = the single ones"""
    import torch
    n, batch, stride = 1 << log2n, 5, (1 << log2n) + 24
    co = noncanonical(oracle.random_scalars(NTT_SEED + 77 + log2n, batch * stride), FR_MODULUS)
    for kind in ("fft", "coset_fft", "ifft_with_constant", "coset_ifft", "coset_fft_with_constant"):
        d = torch.from_numpy(co.view(np.int64)).cuda()
        gpu.ntt_device_batch(d.data_ptr(), n, batch, kind, const, stride=stride)
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(np.uint64)
        for j in range(batch):
            want = oracle.ntt(co[j * stride:j * stride + n], kind, const)
            assert np.array_equal(got[j * stride:j * stride + n], want), (log2n, kind, j)
            assert np.array_equal(got[j * stride + n:(j + 1) * stride], co[j * stride + n:(j + 1) * stride])  # the gap is untouched


def test_ntt_golden_small(gpu, golden):
    g = golden("ntt.json")
    c = limbs(g["constant"])
    for case in g["small"]:
        co = limbs(case["input"]).reshape(-1, 4)
        got = gpu.ntt(co.copy(), case["kind"], c)
        assert np.array_equal(got.reshape(-1), limbs(case["output"])), (case["n"], case["kind"])


@pytest.mark.parametrize("log2n", [8, 10, 12, 16, 20, 22])
def test_ntt_golden_digests(gpu, oracle, golden, log2n):
    """outputs of the reference itself (oracle/_ref) at BASELINE sizes 2^20 and 4*2^20: sha256 + sampled elements"""
    g = golden("ntt.json")
    c = limbs(g["constant"])
    n = 1 << log2n
    co = noncanonical(oracle.random_scalars(NTT_SEED, n), FR_MODULUS)
    for case in [x for x in g["large"] if x["n"] == n]:
        got = gpu.ntt(co.copy(), case["kind"], c)
        for i, v in case["samples"].items():
            assert np.array_equal(got[int(i)], limbs(v)), (log2n, case["kind"], i)
        assert sha(got) == case["sha256"], (log2n, case["kind"])


@pytest.mark.parametrize("log2n", [23, 24])
def test_ntt_golden_digests_extended_domain_sizes(gpu, oracle, golden, log2n):
    """outputs of the reference itself at 2^23 and 2^24 (tests/golden/big_r4.json, tools/gen_golden_r4b.py): the 4n coset domain of a 2^21 /
    2^22-gate circuit; all seven kinds, sha256 + sampled elements"""
    g = golden("big_r4.json")
    c = limbs(g["constant"])
    n = 1 << log2n
    co = noncanonical(oracle.random_scalars(NTT_SEED, n), FR_MODULUS)
    cases = [x for x in g["ntt"] if x["n"] == n]
    assert len(cases) == 7
    for case in cases:
        got = gpu.ntt(co.copy(), case["kind"], c)
        for i, v in case["samples"].items():
            assert np.array_equal(got[int(i)], limbs(v)), (log2n, case["kind"], i)
        assert sha(got) == case["sha256"], (log2n, case["kind"])
        del got


def test_ntt_fft_matches_direct_evaluation(gpu, oracle):
    """test_polynomial_arithmetic.cpp:31-56"""
    n = 16
    poly = oracle.random_scalars(4242, n)
    out = gpu.fft(poly.copy())
    root = oracle.root_of_unity(4)
    w = oracle.const(FR, "one")
    for i in range(n):
        assert np.array_equal(out[i], oracle.evaluate(poly, w))
        w = oracle.mul(FR, w, root)


@pytest.mark.parametrize("log2n", [14, 20, 22])
def test_ntt_roundtrips_full_size(gpu, oracle, log2n):
    """test_polynomial_arithmetic.cpp:58-128 at BASELINE sizes: ifft(fft(x)) == x, coset_ifft(coset_fft(x)) == x"""
    n = 1 << log2n
    x = oracle.random_scalars(99 + log2n, n)  # canonical
    y = gpu.ifft(gpu.fft(x.copy()))
    assert np.array_equal(x, y)
    y = gpu.coset_ifft(gpu.coset_fft(x.copy()))
    assert np.array_equal(x, y)


def test_ntt_cross_domain_coset_consistency(gpu, oracle):
    """test_polynomial_arithmetic.cpp:130-175: coset FFTs of one polynomial on n, 2n, 4n agree on shared points"""
    n = 1 << 10
    base = oracle.random_scalars(777, n)
    outs = []
    for mult in (1, 2, 4):
        buf = np.zeros((mult * n, 4), dtype=np.uint64)
        buf[:n] = base
        outs.append(gpu.coset_fft(buf))
    assert np.array_equal(outs[0], outs[1][::2]) and np.array_equal(outs[0], outs[2][::4])


def test_ntt_linearity_full_size(gpu, oracle):
    n = 1 << 20
    a = oracle.random_scalars(1, n)
    b = oracle.random_scalars(2, n)
    # a + b mod r, vectorised on limbs via python ints would be slow: use fft(a)+fft(b) check on samples instead
    fa, fb = gpu.fft(a.copy()), gpu.fft(b.copy())
    s = np.stack([oracle.add(FR, a[i], b[i]) for i in range(0, n, 1 << 12)])
    full = a.copy()
    for k, i in enumerate(range(0, n, 1 << 12)):
        full[i] = s[k]
    # sparse difference d = full - a is non-zero only at stride 2^12 => fft(full) - fft(a) == fft(d)
    d = np.zeros_like(a)
    for k, i in enumerate(range(0, n, 1 << 12)):
        d[i] = b[i]
    fd, ff = gpu.fft(d.copy()), gpu.fft(full.copy())
    for i in (0, 1, 12345, n - 1):
        assert np.array_equal(ff[i], oracle.add(FR, fa[i], fd[i]))


def test_ntt_three_pass_vs_oracle(gpu, oracle, const):
    """n = 2^23: above the two-pass limit (three HBM passes: columns in place, then batched row transforms); the pre-scaled and the
    post-scaled variant (plain fft / ifft are covered by the next test)"""
    n = 1 << 23
    co = noncanonical(oracle.random_scalars(NTT_SEED + 23, n), FR_MODULUS)
    for kind in ("coset_fft_with_constant", "coset_ifft"):
        want = oracle.ntt(co, kind, const)
        got = gpu.ntt(co.copy(), kind, const)
        assert np.array_equal(got, want), kind


def test_ntt_three_pass_consistent_with_two_pass_and_direct_evaluation(gpu, oracle):
    """2^24: (i) the transform of a zero-padded 2^22-coefficient polynomial on the 4x larger domain agrees with the two-pass 2^22 transform
    on the shared points (test_polynomial_arithmetic.cpp:130-175 at the largest sizes), (ii) sampled outputs equal Horner evaluation at
    w^k, (iii) ifft(fft(x)) == x and coset_ifft(coset_fft(x)) == x"""
    n = 1 << 22
    base = oracle.random_scalars(2424, n)
    small = gpu.fft(base.copy())
    buf = np.zeros((4 * n, 4), dtype=np.uint64)
    buf[:n] = base
    big = gpu.fft(buf.copy())
    assert np.array_equal(big[::4], small)
    root = oracle.root_of_unity(24)
    for k in (1, 3, (1 << 23) + 5, (1 << 24) - 1):
        w = oracle.const(FR, "one")
        b, e = root, k
        while e:  # w = root^k
            if e & 1:
                w = oracle.mul(FR, w, b)
            b = oracle.mul(FR, b, b)
            e >>= 1
        assert np.array_equal(big[k], oracle.evaluate(base, w)), k
    x = oracle.random_scalars(2425, 4 * n)
    assert np.array_equal(gpu.ifft(gpu.fft(x.copy())), x)
    assert np.array_equal(gpu.coset_ifft(gpu.coset_fft(x.copy())), x)


def test_ntt_rejects_bad_sizes(gpu):
    from barretenberg_amd import BbGpuError
    with pytest.raises(BbGpuError):
        gpu.fft(np.zeros((3, 4), dtype=np.uint64))
    with pytest.raises(BbGpuError):
        gpu.fft(np.zeros((1, 4), dtype=np.uint64))


# ------------------------------------------------------------------ MSM ----------------------------------------------
@pytest.fixture(scope="module")
def msm_small(oracle, golden):
    g = golden("msm.json")
    x = limbs(g["srs_secret_mont"])
    n = 1 << 16
    srs = oracle.make_srs(x, n)
    assert sha(srs) == g["srs_digest_65536"]
    table = oracle.point_table(srs)
    scalars = oracle.random_scalars(SCALAR_SEED, n)
    return g, srs, table, scalars


def _check(out, case):
    if "infinity" in case:
        assert bool(int(out[7]) >> 63) == case["infinity"]
    else:
        assert np.array_equal(out[0:4], limbs(case["x"])) and np.array_equal(out[4:8], limbs(case["y"])), case
        assert not (int(out[7]) >> 63)


def test_msm_golden(gpu, oracle, msm_small):
    """normalised results of the reference's pippenger()/batched_scalar_multiplications() on the same inputs"""
    g, srs, table, scalars = msm_small
    one = oracle.const(FQ, "one")
    done = 0
    for case in g["cases"]:
        n = case["n"]
        if n > (1 << 16) or "scalars" in case or "points" in case:
            continue
        out = gpu.pippenger(scalars, table, n)
        _check(out, case)
        if "x" in case:
            assert np.array_equal(out[8:12], one)
        done += 1
    assert done >= 12


def test_msm_edge_cases(gpu, oracle, msm_small):
    g, srs, table, scalars = msm_small
    for case in g["cases"]:
        if case.get("scalars") == "even-index scalars zero":
            zs = scalars[:64].copy()
            zs[::2] = 0
            _check(gpu.pippenger(aligned_copy(zs), table, 64), case)
        elif case.get("scalars") == "all zero":
            _check(gpu.pippenger(aligned_copy(np.zeros((16, 4), dtype=np.uint64)), table, 16), case)
        elif case["n"] == 0:
            _check(gpu.pippenger(scalars, table, 0), case)
        elif "points" in case:
            same_t = oracle.point_table(aligned_copy(np.tile(srs[5], (32, 1))))
            sc = aligned_copy(np.tile(oracle.const(FR, "one"), (32, 1))) if case.get("scalars") == "all one" else scalars
            _check(gpu.pippenger(sc, same_t, 32), case)


def test_msm_noncanonical_scalars(gpu, oracle, msm_small):
    """scalars in [r, 2r) (kate coefficients, polynomial_arithmetic.cpp:580-588) give the same point"""
    g, srs, table, scalars = msm_small
    n = 1000
    sc = noncanonical(scalars[:n], FR_MODULUS)
    case = [c for c in g["cases"] if c["n"] == 1000][0]
    _check(gpu.pippenger(aligned_copy(sc), table, n), case)


def test_msm_batched(gpu, oracle, msm_small):
    """scalar_multiplication.cpp:650-772 / test_scalar_multiplication.cpp:271-324"""
    g, srs, table, scalars = msm_small
    big = oracle.random_scalars(SCALAR_SEED, 3 * 4096)
    jobs = [(table, aligned_copy(big[o:o + 4096]), 4096) for o in (0, 4096, 8192)]
    outs = gpu.batched_scalar_multiplications(jobs)
    for out, want in zip(outs, g["batched_3x4096"]):
        assert np.array_equal(out[0:4], limbs(want["x"])) and np.array_equal(out[4:8], limbs(want["y"]))
        assert np.array_equal(out[8:12], limbs(want["z"]))
    from barretenberg_amd import BbGpuError
    with pytest.raises(BbGpuError):
        gpu.batched_scalar_multiplications([(table, scalars, 8), (table, scalars, 9)])


def test_msm_subslice_of_registered_table(gpu, oracle, msm_small):
    """batched_scalar_multiplications hands pippenger sub-slices points + 2*off of one table (:720-726)"""
    g, srs, table, scalars = msm_small
    off, n = 100, 300
    want = oracle.msm_affine(aligned_copy(scalars[off:off + n]), aligned_copy(table[2 * off:2 * (off + n)]), n)
    h = gpu.srs_register(table)
    got = gpu.pippenger(aligned_copy(scalars[off:off + n]), table[2 * off:], n)
    assert np.array_equal(got[:8], want[:8])
    assert gpu.srs_register(table) == h


def test_msm_vs_oracle_random_sizes(gpu, oracle, msm_small):
    g, srs, table, scalars = msm_small
    for n in (5, 31, 257, 2048):
        want = oracle.msm_affine(scalars, table, n)
        assert np.array_equal(gpu.pippenger(scalars, table, n)[:8], want[:8]), n


def test_msm_window_sharding_adds_up(gpu, oracle, msm_small):
    """multi-GPU path on one device: partial sums over disjoint window ranges fold to the full MSM (bbgpu_g1_sum)"""
    import torch
    g, srs, table, scalars = msm_small
    n = 1 << 14
    h = gpu.srs_register(table)
    d_sc = torch.from_numpy(scalars[:n].view(np.int64)).cuda()
    W = gpu.srs_num_windows(h, n)
    full = gpu.msm_device(h, d_sc.data_ptr(), n)
    want = oracle.msm_affine(scalars, table, n)
    assert np.array_equal(full[:8], want[:8])
    for parts in (2, 4, 8):
        bounds = [W * r // parts for r in range(parts + 1)]
        partials = [gpu.msm_device(h, d_sc.data_ptr(), n, 0, bounds[r], bounds[r + 1]) for r in range(parts) if bounds[r] < bounds[r + 1]]
        assert np.array_equal(gpu.g1_sum(np.stack(partials)), full), parts


def test_msm_skewed_scalars(gpu, oracle, msm_small):
    """digit distributions far from uniform (what real witnesses look like): every scalar equal, scalars in {0, 1, -1},
    tiny scalars -- exercises the heavy-bucket merge path (one bucket cut into thousands of chunk partials)"""
    g, srs, table, scalars = msm_small
    n = 1 << 14
    one = oracle.const(FR, "one")
    minus_one = oracle.neg(FR, one)
    rng = np.random.default_rng(5)
    sets = {
        "all equal": np.tile(scalars[7], (n, 1)),
        "0/1/-1": np.stack([(np.zeros(4, dtype=np.uint64), one, minus_one)[i] for i in rng.integers(0, 3, n)]),
        "small": np.stack([oracle.to_mont(FR, np.array([int(v), 0, 0, 0], dtype=np.uint64)) for v in rng.integers(0, 200, n)]),
    }
    for name, sc in sets.items():
        sc = aligned_copy(sc)
        want = oracle.msm_affine(sc, table, n)
        got = gpu.pippenger(sc, table, n)
        assert np.array_equal(got[:8], want[:8]), name
        assert (int(got[7]) >> 63) == (int(want[7]) >> 63), name


def test_msm_fuzz_sizes_and_distributions(gpu, oracle, msm_small):
    """48 seeded cases against the oracle: sizes with every residue mod 8 on both sides of the window-table threshold (n % 8 == 0 takes the
    16-byte digit loads and the LDS-staged sort passes, the rest the one-digit-per-load kernels; below 1024 points one bucket set per
    window), scalar mixtures from uniform to degenerate (zeros, +-1, one repeated value, 20-bit values, a single non-zero scalar)"""
    g, srs, table, scalars = msm_small
    one = oracle.const(FR, "one")
    minus_one = oracle.neg(FR, one)
    zero = np.zeros(4, dtype=np.uint64)
    rng = np.random.default_rng(20260402)
    sizes = [25, 26, 63, 64, 200, 1000, 1023, 1024, 1025, 1032, 2047, 2048, 2056, 3001, 4096, 5000]
    for case in range(48):
        n = sizes[case % len(sizes)] + (int(rng.integers(0, 8)) if case >= 32 else 0)
        kind = case % 6
        sc = scalars[case * 5: case * 5 + n].copy()
        if kind == 1:    # a third zeros, a third +-1
            pick = rng.integers(0, 4, n)
            sc[pick == 0] = zero
            sc[pick == 1] = one
            sc[pick == 2] = minus_one
        elif kind == 2:  # one value everywhere
            sc[:] = scalars[case]
        elif kind == 3:  # 20-bit values
            sc = np.stack([oracle.to_mont(FR, np.array([int(v), 0, 0, 0], dtype=np.uint64)) for v in rng.integers(0, 1 << 20, n)])
        elif kind == 4:  # a single non-zero scalar
            keep = int(rng.integers(0, n))
            v = sc[keep].copy()
            sc[:] = zero
            sc[keep] = v
        elif kind == 5:  # runs of repeated values (what selector-like witnesses look like)
            sc = np.repeat(scalars[case: case + (n + 15) // 16], 16, axis=0)[:n].copy()
        sc = aligned_copy(sc)
        want = oracle.msm_affine(sc, table, n)
        got = gpu.pippenger(sc, table, n)
        assert (int(got[7]) >> 63) == (int(want[7]) >> 63), (case, n, kind)
        if not (int(want[7]) >> 63):
            assert np.array_equal(got[:8], want[:8]), (case, n, kind)


def test_msm_additivity_large(gpu, oracle):
    """sizes beyond the round-1 fixtures (non-power-of-two, and 2^21 = two window-table segments, or per-window bucket sets in the no-tables pass):
    MSM(n) == MSM(first half) + MSM(second half), through independent code paths (different n => different chunking; the cut is not the segment
    boundary).  Reference points for 2^21 and 2^20 + 8: test_msm_beyond_one_table_segment."""
    import torch
    x = oracle.random_scalars(SRS_SEED + 1, 1)[0]
    for n in (3 << 18, 1 << 21):
        h = gpu.srs_generate(x, n)
        sc = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64(0x1FFFFFFFFFFFFFFF)
        d = torch.from_numpy(sc.view(np.int64)).cuda()
        full = gpu.msm_device(h, d.data_ptr(), n)
        m = n // 2 + 12345
        lo = gpu.msm_device(h, d.data_ptr(), m)
        hi = gpu.msm_device(h, d.data_ptr() + m * 32, n - m, offset=m)
        assert np.array_equal(gpu.g1_sum(np.stack([lo, hi])), full), n
        assert not (int(full[7]) >> 63)
        gpu.srs_release(h)


def test_msm_small_unregistered_tables_are_not_cached(gpu, oracle, msm_small):
    """the verifier builds a fresh ~20-point table per proof (verifier.cpp:359-363): the same host buffer refilled with OTHER points
    must give the new result (no stale resident copy keyed by the address), call after call"""
    g, srs, table, scalars = msm_small
    n = 24
    buf = aligned_copy(table[:2 * n])
    sc = aligned_copy(scalars[:n])
    first = gpu.pippenger(sc, buf, n)
    assert np.array_equal(first[:8], oracle.msm_affine(sc, aligned_copy(table[:2 * n]), n)[:8])
    buf[...] = table[2 * 100:2 * 100 + 2 * n]  # same address, different points
    second = gpu.pippenger(sc, buf, n)
    assert np.array_equal(second[:8], oracle.msm_affine(sc, aligned_copy(table[200:200 + 2 * n]), n)[:8])
    assert not np.array_equal(first, second)
    for _ in range(50):  # and no per-call registration piling up
        assert np.array_equal(gpu.pippenger(sc, buf, n), second)


def test_msm_device_batch(gpu, oracle, msm_small):
    """whole-batch entry: up to four scalar vectors over the same points in one pass = the single MSMs, including
    an all-zero vector, a skewed one, and sub-ranges of the registered table"""
    import torch
    from barretenberg_amd import BbGpuError
    g, srs, table, scalars = msm_small
    h = gpu.srs_register(table)
    one = oracle.to_mont(FR, np.array([1, 0, 0, 0], dtype=np.uint64))
    for n in (16, 1000, 4096, 65536):
        sets = [scalars[:n], scalars[::-1][:n].copy(), np.zeros((n, 4), dtype=np.uint64), np.tile(one, (n, 1))]
        dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in sets]
        single = [gpu.msm_device(h, d.data_ptr(), n) for d in dev]
        assert oracle.is_infinity(single[2]) and not oracle.is_infinity(single[0])
        for jobs in (1, 2, 3, 4):
            try:
                t = gpu.msm_device_batch_async(h, [d.data_ptr() for d in dev[:jobs]], n)
            except BbGpuError:
                assert jobs > 1  # no window tables on this SRS (the no-tables parametrisation): refused, callers fall back
                continue
            got = gpu.msm_batch_wait(t)
            for j in range(jobs):
                assert np.array_equal(got[j], single[j]), (n, jobs, j)
    # a sub-range of the table
    n, off = 3000, 777
    d = torch.from_numpy(scalars[:n].view(np.int64)).cuda()
    want = gpu.msm_device(h, d.data_ptr(), n, offset=off)
    try:
        got = gpu.msm_batch_wait(gpu.msm_device_batch_async(h, [d.data_ptr(), d.data_ptr()], n, offset=off))
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    except BbGpuError:
        pass


def test_msm_async_pipeline(gpu, oracle, msm_small):
    """two MSMs in flight (bbgpu_msm_g1_device_async / _wait): results independent of the overlap"""
    import torch
    from barretenberg_amd import BbGpuError
    g, srs, table, scalars = msm_small
    h = gpu.srs_register(table)
    sizes = [4096, 1000, 65536, 16, 10000]
    d = {n: torch.from_numpy(scalars[:n].view(np.int64)).cuda() for n in sizes}
    want = {n: [c for c in g["cases"] if c["n"] == n and "x" in c][0] for n in sizes}
    inflight, got = [], []
    for n in sizes + sizes:
        inflight.append((n, gpu.msm_device_async(h, d[n].data_ptr(), n)))
        if len(inflight) == 2:
            m, t = inflight.pop(0)
            got.append((m, gpu.msm_wait(t)))
    with pytest.raises(BbGpuError):  # one is still in flight and there are eight slots: the eighth extra enqueue must be refused
        for _ in range(8):
            gpu.msm_device_async(h, d[16].data_ptr(), 16)
    while inflight:
        m, t = inflight.pop(0)
        got.append((m, gpu.msm_wait(t)))
    # drain whatever the failed double-issue left behind
    for t in range(8):
        try:
            gpu.msm_wait(t)
        except BbGpuError:
            pass
    assert len(got) == 10
    for m, out in got:
        _check(out, want[m])


def test_srs_generate_and_msm_2_20(gpu, oracle, golden):
    """BASELINE config 2: 2^20-point MSM, random scalars vs the synthetic SRS; expected point from the reference."""
    import torch
    g = golden("msm.json")
    n = 1 << 20
    x = limbs(g["srs_secret_mont"])
    h, table = gpu.srs_generate(x, n, want_host_table=True)
    for i, v in g["srs_samples"].items():
        assert np.array_equal(table[2 * int(i)], limbs(v))
    assert sha(table[0:2 * 65536:2]) == g["srs_digest_65536"]
    assert sha(table[0::2]) == g["srs_digest_1048576"]
    assert sha(table[:8192]) == g["table_digest_4096"]  # endo entries too
    scalars = oracle.random_scalars(SCALAR_SEED, n)
    d_sc = torch.from_numpy(scalars.view(np.int64)).cuda()
    out = gpu.msm_device(h, d_sc.data_ptr(), n)
    case = [c for c in g["cases"] if c["n"] == n][0]
    _check(out, case)
    # host-pointer path resolves to the same resident table
    out2 = gpu.pippenger(scalars, table, n)
    assert np.array_equal(out, out2)
    # BASELINE config 4 at full size on one GPU: the 8-way split the driver runs across 8 ranks -- eight shares of whole digit
    # windows and (against window tables) eight row-range shares [W n r / 8, W n (r + 1) / 8) -- folded with bbgpu_g1_sum
    W = gpu.srs_num_windows(h, n)
    bounds = [W * r // 8 for r in range(9)]
    parts = [gpu.msm_device(h, d_sc.data_ptr(), n, 0, a, b) for a, b in zip(bounds[:-1], bounds[1:]) if a < b]
    _check(gpu.g1_sum(np.stack(parts)), case)
    if gpu.srs_has_window_tables(h):
        R = W * n
        cuts = [R * r // 8 for r in range(9)]
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):  # two in flight, like the ranks' pipelines
            parts.append(gpu.msm_wait(gpu.msm_device_rows_async(h, d_sc.data_ptr(), n, a, b)))
        _check(gpu.g1_sum(np.stack(parts)), case)
        # ... and eight (and three: 256 rows of the bucket matrix do not divide by 3) BUCKET-range shares: every share over all windows
        # and points, 1 / N of the buckets each (round 3: the split whose per-rank tail shrinks with N)
        for N in (8, 3):
            tickets, parts = [], []
            for r in range(N):  # two in flight
                tickets.append(gpu.msm_device_buckets_async(h, d_sc.data_ptr(), n, r, N))
                if len(tickets) == 2:
                    parts.append(gpu.msm_wait(tickets.pop(0)))
            parts += [gpu.msm_wait(t) for t in tickets]
            _check(gpu.g1_sum(np.stack(parts)), case)
    # ... and the POINT-range split (bench.py --shard points, the default from round 3 on): rank r holds points and scalars
    # [n r / N, n (r + 1) / N) as its own SRS (bbgpu_set_point_share + bbgpu_srs_generate_range), all digit windows; four in flight, so the shares
    # after the first take the throughput choices (longer chunks, two-step row / column sums).  N = 8 and N = 3 (uneven ranges).
    for N in (8, 3):
        cuts = [n * r // N for r in range(N + 1)]
        gpu.set_point_share(N)
        slices = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            hs, ts = gpu.srs_generate(x, b - a, want_host_table=True, first=a)
            assert np.array_equal(ts, table[2 * a:2 * b])  # the slice IS that range of the whole table
            slices.append(hs)
        gpu.set_point_share(1)
        tickets, parts = [], []
        for r, hs in enumerate(slices):
            tickets.append(gpu.msm_device_async(hs, d_sc.data_ptr() + cuts[r] * 32, cuts[r + 1] - cuts[r]))
            if len(tickets) == 4:
                parts.append(gpu.msm_wait(tickets.pop(0)))
        parts += [gpu.msm_wait(t) for t in tickets]
        _check(gpu.g1_sum(np.stack(parts)), case)
        # the same ranges of the WHOLE table (offset calls), two in flight
        tickets, parts2 = [], []
        for r in range(N):
            tickets.append(gpu.msm_device_async(h, d_sc.data_ptr() + cuts[r] * 32, cuts[r + 1] - cuts[r], cuts[r]))
            if len(tickets) == 2:
                parts2.append(gpu.msm_wait(tickets.pop(0)))
        parts2 += [gpu.msm_wait(t) for t in tickets]
        assert np.array_equal(np.stack(parts), np.stack(parts2))
        for hs in slices:
            gpu.srs_release(hs)


def test_msm_bucket_range_shares(gpu, oracle, msm_small, golden):
    """bucket-range shares (bbgpu_msm_g1_device_buckets_async) against the oracle: sizes on both sides of the 16-byte digit loads
    (n % 8 != 0 takes the one-digit-per-load sort kernels), share counts that do and do not divide the bucket matrix's rows, uniform
    and skewed scalars (all equal: whole windows fall into ONE share, the others see empty lists; {0, 1, -1}; small values) -- the
    shares of one MSM must add up to the oracle's point, and a single share of one must equal the MSM itself"""
    import torch
    g, srs, table, scalars = msm_small
    one = oracle.const(FR, "one")
    minus_one = oracle.neg(FR, one)
    rng = np.random.default_rng(11)
    for n in (1 << 14, 5000, 1029):
        tab = aligned_copy(table[:2 * n])
        h = gpu.srs_register(tab)
        if not gpu.srs_has_window_tables(h):  # the suite's second pass (bbgpu_set_precompute(0)): shares of the bucket range need the shared bucket set
            from barretenberg_amd import BbGpuError
            d0 = torch.from_numpy(aligned_copy(scalars[:n]).view(np.int64)).cuda()
            with pytest.raises(BbGpuError):
                gpu.msm_device_buckets_async(h, d0.data_ptr(), n, 0, 2)
            gpu.srs_release(h)
            continue
        sets = {
            "uniform": scalars[:n],
            "all equal": np.tile(scalars[7], (n, 1)),
            "0/1/-1": np.stack([(np.zeros(4, dtype=np.uint64), one, minus_one)[i] for i in rng.integers(0, 3, n)]),
            "small": np.stack([oracle.to_mont(FR, np.array([int(v), 0, 0, 0], dtype=np.uint64)) for v in rng.integers(0, 200, n)]),
        }
        for name, sc in sets.items():
            sc = aligned_copy(sc)
            want = oracle.msm_affine(sc, tab, n)
            d = torch.from_numpy(sc.view(np.int64)).cuda()
            for N in (1, 2, 5, 8):
                parts = [gpu.msm_wait(gpu.msm_device_buckets_async(h, d.data_ptr(), n, r, N)) for r in range(N)]
                got = gpu.g1_sum(np.stack(parts))
                assert np.array_equal(got[:8], want[:8]), (n, name, N)
        gpu.srs_release(h)
    # argument checks: share out of range, more shares than rows of the bucket matrix, a table without window tables
    from barretenberg_amd import BbGpuError
    tab = aligned_copy(table[:2 * 2048])
    h = gpu.srs_register(tab)
    d = torch.from_numpy(aligned_copy(scalars[:2048]).view(np.int64)).cuda()
    for share, count in ((2, 2), (-1, 2), (0, 0), (0, 100000)):
        with pytest.raises(BbGpuError):
            gpu.msm_device_buckets_async(h, d.data_ptr(), 2048, share, count)
    gpu.srs_release(h)
    gpu.set_precompute(False)
    try:
        h = gpu.srs_register(tab)
        with pytest.raises(BbGpuError):
            gpu.msm_device_buckets_async(h, d.data_ptr(), 2048, 0, 2)
        gpu.srs_release(h)
    finally:
        gpu.set_precompute(True)


def test_msm_around_the_table_mode_switch(gpu, oracle, golden):
    """n = 2^19 - 8, 2^19, 2^19 + 8, 3 * 2^18: both sides of the window-table switch (capi.hip add_srs: 15-bit windows below 2^19, 17-bit
    from there on) against points the REFERENCE computed for exactly these prefixes (tests/golden/msm_r3.json, tools/gen_golden_r3.py)"""
    import torch
    g = golden("msm_r3.json")
    x = limbs(g["srs_secret_mont"])
    scalars = oracle.random_scalars(SCALAR_SEED, 3 << 18)
    d_sc = torch.from_numpy(scalars.view(np.int64)).cuda()
    for case in g["threshold"]:
        n = case["n"]
        if n == 3 << 18:
            # the same through the HOST-pointer entry (bbgpu_msm_g1): from 2^19 points on it runs as two point ranges (3/8 + 5/8 of the
            # points, the second range's scalars crossing the link under the first one's kernels) whose partial sums are added on the host
            h, table = gpu.srs_generate(x, n, True)
            _check(gpu.pippenger(aligned_copy(scalars[:n]), table, n), case)
            for m in ((1 << 19) + 8, 1 << 19, (1 << 19) - 8):  # prefixes of the same table: two ranges, two ranges, one range
                _check(gpu.pippenger(aligned_copy(scalars[:m]), table, m), [c for c in g["threshold"] if c["n"] == m][0])
        else:
            h = gpu.srs_generate(x, n)
        _check(gpu.msm_device(h, d_sc.data_ptr(), n), case)
        # a prefix of a LARGER table keeps that table's window size: the 2^19 - 8 prefix on 17-bit tables, too
        if n == (1 << 19) + 8:
            _check(gpu.msm_device(h, d_sc.data_ptr(), (1 << 19) - 8), [c for c in g["threshold"] if c["n"] == (1 << 19) - 8][0])
        gpu.srs_release(h)


def test_msm_beyond_one_table_segment(gpu, oracle, golden):
    """n > 2^20: the SRS keeps one window table per <= 2^20-point segment (capi.hip add_srs) and an MSM runs as point-range pieces -- dealt to the
    ticket's slot and a helper slot, piece sums added on the host -- instead of falling back to per-window bucket sets.  Points the REFERENCE
    computed for prefixes of a 2^21-point SRS (tests/golden/msm_r4.json, tools/gen_golden_r4.py): 2^19 + 3 (ragged, two ranges at the host entry,
    ADVICE r3), 2^20 + 8 and 2^21 (two segments), and scalars[0:n] against points [5, 5 + n) (a sub-slice across the segment boundary), through
    the device entry, the host-pointer entries, the batched entry and two compound tickets in flight."""
    import torch
    g = golden("msm_r4.json")
    x = limbs(g["srs_secret_mont"])
    N = 1 << 21
    h, table = gpu.srs_generate(x, N, True)
    assert sha(table[0::2]) == g["srs_digest_2097152"]
    scalars = oracle.random_scalars(SCALAR_SEED, N)
    d_sc = torch.from_numpy(scalars.view(np.int64)).cuda()
    for case in g["prefixes"]:
        n = case["n"]
        _check(gpu.msm_device(h, d_sc.data_ptr(), n), case)
        _check(gpu.pippenger(aligned_copy(scalars[:n]), table, n), case)  # host pointers: served from the resident copy of `table`
    n = g["prefixes"][0]["n"]  # 2^19 + 3 on the PLAIN n-entry table (pippenger_low_memory): used once, its own upload, two ragged ranges
    _check(gpu.pippenger_low_memory(aligned_copy(scalars[:n]), aligned_copy(table[0:2 * n:2]), n), g["prefixes"][0])
    sl = g["slice"]
    _check(gpu.msm_device(h, d_sc.data_ptr(), sl["n"], offset=sl["offset"]), sl)
    _check(gpu.pippenger(aligned_copy(scalars[:sl["n"]]), table[2 * sl["offset"]:], sl["n"]), sl)
    full = g["prefixes"][-1]
    # two tickets of 2^21 points in flight (each in two pieces; the first takes a helper slot, the second whatever is left)
    t1, t2 = gpu.msm_device_async(h, d_sc.data_ptr(), N), gpu.msm_device_async(h, d_sc.data_ptr(), N)
    _check(gpu.msm_wait(t2), full)
    _check(gpu.msm_wait(t1), full)
    if gpu.srs_has_window_tables(h):
        assert gpu.srs_num_windows(h, N) == 15
        # the batched entry over two segments: three jobs in one pass per piece
        rev = torch.from_numpy(np.ascontiguousarray(scalars[::-1]).view(np.int64)).cuda()
        got = gpu.msm_batch_wait(gpu.msm_device_batch_async(h, [d_sc.data_ptr(), rev.data_ptr(), d_sc.data_ptr()], N))
        _check(got[0], full)
        _check(got[2], full)
        assert np.array_equal(got[1], gpu.msm_device(h, rev.data_ptr(), N))
        # row / bucket shares are defined on ONE table segment: refused here (a larger MSM is split by point range)
        from barretenberg_amd import BbGpuError
        with pytest.raises(BbGpuError, match="ONE table segment"):
            gpu.msm_device_rows_async(h, d_sc.data_ptr(), N, 0, N)
    gpu.srs_release(h)


def test_msm_host_batch_jobs_straddling_a_segment_boundary(gpu, oracle, golden):
    """batched_scalar_multiplications() (bbgpu_msm_g1_batch) with jobs of 2^19 points that start 2^18 (- 11 k) points before the boundary between the two
    window-table segments of a 2^21-point SRS: every job runs as two pieces, the second one on a HELPER slot whose stream must wait for the
    scalars' asynchronous upload on the job's own stream (16 MiB per job, large enough for the digit kernel to overtake the DMA
    were the dependency missing).  Points the REFERENCE computed for exactly these jobs (tests/golden/msm_r5.json, tools/gen_golden_r5.py)."""
    g = golden("msm_r5.json")
    N = 1 << 21
    h, table = gpu.srs_generate(limbs(g["srs_secret_mont"]), N, True)
    assert sha(table[0::2]) == g["srs_digest_2097152"]
    scalars = oracle.random_scalars(SCALAR_SEED, N)
    cases = g["straddle"]
    for rounds in range(2):  # the second round finds the staging buffers and the helper's workspace warm: the upload is then the only thing in front of the kernels
        jobs = [(table[2 * c["offset"]:], aligned_copy(scalars[c["scalars_from"]:c["scalars_from"] + c["n"]]), c["n"]) for c in cases]
        outs = gpu.batched_scalar_multiplications(jobs)
        for c, out in zip(cases, outs):
            _check(out, c)
    # the same jobs one at a time through pippenger() (two ranges per segment piece at the host entry)
    c = cases[1]
    _check(gpu.pippenger(aligned_copy(scalars[c["scalars_from"]:c["scalars_from"] + c["n"]]), table[2 * c["offset"]:], c["n"]), c)
    gpu.srs_release(h)


def test_msm_four_table_segments(gpu, oracle, golden):
    """n = 2^22 and n = 3 * 2^20 + 11 on a 2^22-point SRS (four window-table segments; the ragged size leaves the last one partly used): points the
    REFERENCE computed (tests/golden/big_r4.json, tools/gen_golden_r4b.py), through the device entry, the host-pointer entry and a two-job batch"""
    import torch
    g = golden("big_r4.json")
    N = 1 << 22
    h, table = gpu.srs_generate(limbs(g["srs_secret_mont"]), N, True)
    assert sha(table[0::2]) == g["srs_digest_%d" % N]
    scalars = oracle.random_scalars(SCALAR_SEED, N)
    d_sc = torch.from_numpy(scalars.view(np.int64)).cuda()
    for case in g["msm"]:
        n = case["n"]
        _check(gpu.msm_device(h, d_sc.data_ptr(), n), case)
        _check(gpu.pippenger(aligned_copy(scalars[:n]), table, n), case)
    if gpu.srs_has_window_tables(h):  # the batched entry needs them
        got = gpu.msm_batch_wait(gpu.msm_device_batch_async(h, [d_sc.data_ptr(), d_sc.data_ptr()], N))
        _check(got[0], g["msm"][-1])
        _check(got[1], g["msm"][-1])
    gpu.srs_release(h)


def test_msm_pieces_against_the_oracle(gpu, oracle, msm_small):
    """the piece machinery of the large MSMs (one window table per segment, pieces dealt to the ticket's slot and a helper, piece sums added on the
    host) at sizes the ORACLE checks: BBGPU_TABLE_SEG_POINTS cuts a 10,000-point SRS into 10, 4 and 63 segments (1,000 / 2,504 / 160 points) --
    prefixes, sub-slices that start and end inside segments, batches, window sub-ranges, skewed scalars, three compound tickets in flight (the later
    ones find fewer free helper slots, down to all pieces on one slot), the host-pointer entries"""
    import os
    import torch
    from barretenberg_amd import BbGpuError
    g, srs, table, scalars = msm_small
    n_all = 10000
    one = oracle.const(FR, "one")
    rng = np.random.default_rng(5)
    try:
        for seg in (1000, 3000, 160):
            os.environ["BBGPU_TABLE_SEG_POINTS"] = str(seg)
            tab = aligned_copy(table[:2 * n_all])  # its own address: a fresh registration under this segment size
            h = gpu.srs_register(tab)
            d = torch.from_numpy(aligned_copy(scalars[:n_all]).view(np.int64)).cuda()
            cases = [(0, n_all), (0, seg), (0, seg + 1), (seg - 1, 2), (seg // 2, 2 * seg + 7), (3, n_all - 3), (n_all - 5, 5), (2 * seg, seg)]
            for off, n in cases:
                want = oracle.msm_affine(aligned_copy(scalars[:n]), aligned_copy(table[2 * off:2 * (off + n)]), n)
                got = gpu.msm_device(h, d.data_ptr(), n, offset=off)
                assert np.array_equal(got[:8], want[:8]), (seg, off, n)
                assert np.array_equal(gpu.pippenger(aligned_copy(scalars[:n]), tab[2 * off:], n)[:8], want[:8]), ("host", seg, off, n)
            # the host-pointer batch (batched_scalar_multiplications) over sub-slices that straddle segment boundaries: a straddling job goes through the
            # slot pipeline as one range per segment it touches
            nb = min(2 * seg, 1500)
            offs = [max(0, seg - 5), 3, 2 * seg - nb // 2, seg // 2]
            jobs = [(tab[2 * o:], aligned_copy(scalars[k:k + nb]), nb) for k, o in enumerate(offs)]
            outs = gpu.batched_scalar_multiplications(jobs)
            for k, o in enumerate(offs):
                want = oracle.msm_affine(aligned_copy(scalars[k:k + nb]), aligned_copy(table[2 * o:2 * (o + nb)]), nb)
                assert np.array_equal(outs[k][:8], want[:8]), ("host batch", seg, k, o)
            if gpu.srs_has_window_tables(h):
                W = gpu.srs_num_windows(h, n_all)
                full = gpu.msm_device(h, d.data_ptr(), n_all)
                parts = [gpu.msm_device(h, d.data_ptr(), n_all, window_begin=a, window_end=b) for a, b in ((0, W // 3), (W // 3, W - 1), (W - 1, W))]
                assert np.array_equal(gpu.g1_sum(np.stack(parts)), full), seg
                sets = [scalars[:n_all], np.tile(scalars[7], (n_all, 1)), np.stack([(np.zeros(4, dtype=np.uint64), one)[i] for i in rng.integers(0, 2, n_all)])]
                dev = [torch.from_numpy(aligned_copy(a).view(np.int64)).cuda() for a in sets]
                single = [gpu.msm_device(h, x.data_ptr(), n_all) for x in dev]
                for k, a in enumerate(sets):
                    assert np.array_equal(single[k][:8], oracle.msm_affine(aligned_copy(a), tab, n_all)[:8]), (seg, k)
                got = gpu.msm_batch_wait(gpu.msm_device_batch_async(h, [x.data_ptr() for x in dev], n_all))
                for k in range(3):
                    assert np.array_equal(got[k], single[k]), (seg, "batch", k)
                tickets = [gpu.msm_device_async(h, dev[k % 3].data_ptr(), n_all) for k in range(3)]  # compound tickets: the later ones find fewer free helpers
                for k, t in enumerate(tickets):
                    assert np.array_equal(gpu.msm_wait(t), single[k % 3]), (seg, "in flight", k)
            gpu.srs_release(h)
    finally:
        del os.environ["BBGPU_TABLE_SEG_POINTS"]


@pytest.fixture(scope="module")
def few_slots_wants(oracle, msm_small):
    """oracle points for the two tests below, computed once: the 4096-point MSM the held tickets run, the 10,000-point MSM and three 1,500-point jobs
    whose sub-slices straddle the boundaries of 1,000-point segments"""
    g, srs, table, scalars = msm_small
    offs = (995, 3, 2500)
    return {
        "held": oracle.msm_affine(aligned_copy(scalars[:4096]), aligned_copy(table[:2 * 4096]), 4096),
        "whole": oracle.msm_affine(aligned_copy(scalars[:10000]), aligned_copy(table[:2 * 10000]), 10000),
        "offs": offs,
        "jobs": [oracle.msm_affine(aligned_copy(scalars[k:k + 1500]), aligned_copy(table[2 * o:2 * (o + 1500)]), 1500) for k, o in enumerate(offs)],
    }


def _hold_tickets(gpu, table, scalars, count):
    """`count` asynchronous 4096-point MSMs in flight on a registered table: they keep their slots until msm_wait()"""
    import torch
    h = gpu.srs_register(aligned_copy(table[:2 * 4096]))
    d = torch.from_numpy(aligned_copy(scalars[:4096]).view(np.int64)).cuda()
    return h, d, [gpu.msm_device_async(h, d.data_ptr(), 4096) for _ in range(count)]


def test_msm_host_entries_with_few_free_slots(gpu, msm_small, few_slots_wants):
    """pippenger() and batched_scalar_multiplications() while a caller holds asynchronous tickets: 7 held leave ONE free slot, 6 held leave two that
    are not slots 0 / 1.  The 10,000-point table is cut into ten 1,000-point segments (BBGPU_TABLE_SEG_POINTS), so the single call is ten ranges and
    every job of the batch lies above one segment.  All results equal the oracle's, the held tickets' as well."""
    import os
    g, srs, table, scalars = msm_small
    W = few_slots_wants
    for held in (7, 6):
        h, d, tickets = _hold_tickets(gpu, table, scalars, held)
        assert gpu.fault_stats()["slots_pending"] == held
        try:
            os.environ["BBGPU_TABLE_SEG_POINTS"] = "1000"
            tab = aligned_copy(table[:2 * 10000])  # its own address: registered on first sight under this segment size
            assert np.array_equal(gpu.pippenger(aligned_copy(scalars[:10000]), tab, 10000)[:8], W["whole"][:8]), held
            jobs = [(tab[2 * o:], aligned_copy(scalars[k:k + 1500]), 1500) for k, o in enumerate(W["offs"])]
            outs = gpu.batched_scalar_multiplications(jobs)
            for k in range(3):
                assert np.array_equal(outs[k][:8], W["jobs"][k][:8]), (held, k)
        finally:
            del os.environ["BBGPU_TABLE_SEG_POINTS"]
        assert gpu.fault_stats()["slots_pending"] == held
        for t in tickets:
            assert np.array_equal(gpu.msm_wait(t)[:8], W["held"][:8]), (held, t)
        assert gpu.fault_stats()["slots_pending"] == 0
        gpu.srs_release(h)


def test_msm_batch_null_job_with_one_context(gpu, msm_small, few_slots_wants):
    """three jobs of 2048 points, job 2's scalars null, in ONE context: error -3, nothing left in flight, and the outputs written are those of the
    jobs collected by the time job 2 is looked at -- job 0 with all slots free (job 1 is still in flight on the second slot), jobs 0 and 1 with one
    free slot (7 tickets held).  The text carries the job number where two slots are free, "null scalars/points in job 2"; with one free slot it is
    the plain "null scalars/points".  That is the parent commit's text, learnt by running this test once against the parent's library (there such a
    batch ran job by job through the single-call entry), which passes it whole.  With no slot free and job 0 null it is still the null job that is
    reported, nothing written, the 8 tickets held."""
    import ctypes as C
    from barretenberg_amd.bbgpu import MsmJob, _ptr
    g, srs, table, scalars = msm_small
    n = 2048
    t = aligned_copy(table[:2 * n])
    sc = [aligned_copy(scalars[k * n:(k + 1) * n]) for k in range(3)]
    want = [gpu.pippenger(s, t, n) for s in sc[:2]]

    def run(null=2):
        arr = (MsmJob * 3)()
        for j, s in zip(arr, sc):
            j.points, j.scalars, j.num_elements = _ptr(t), _ptr(s), n
        arr[null].scalars = C.cast(None, type(arr[null].scalars))
        rc = gpu.lib.bbgpu_msm_g1_batch(arr, 3)
        return rc, gpu.lib.bbgpu_last_error().decode(), [np.array(list(j.output), dtype=np.uint64) for j in arr]

    rc, text, out = run()
    print("all slots free:", rc, repr(text))
    assert rc == -3 and text == "null scalars/points in job 2"
    assert np.array_equal(out[0], want[0])
    assert not out[1].any() and not out[2].any()
    assert gpu.fault_stats()["slots_pending"] == 0
    h, d, tickets = _hold_tickets(gpu, table, scalars, 7)
    rc, text, out = run()
    print("one slot free:", rc, repr(text))
    assert rc == -3 and text == "null scalars/points"
    assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])
    assert not out[2].any()
    assert gpu.fault_stats()["slots_pending"] == 7
    tickets.append(gpu.msm_device_async(h, d.data_ptr(), 4096))  # no slot free: a null job 0 is still reported as such, its pointers come before the slots
    rc, text, out = run(null=0)
    print("no slot free, job 0 null:", rc, repr(text))
    assert rc == -3 and text == "null scalars/points"
    assert not any(o.any() for o in out)
    assert gpu.fault_stats()["slots_pending"] == 8
    for tk in tickets:
        assert np.array_equal(gpu.msm_wait(tk)[:8], few_slots_wants["held"][:8])
    gpu.srs_release(h)


def test_msm_skewed_scalars_full_size(gpu, oracle, golden):
    """the skewed scalar sets (every scalar equal, {0, 1, -1}, values below 200: bench.skewed_scalars) at the FULL 2^20 size -- the
    heavy-bucket merge path at the size the headline is quoted on -- against the reference's points for the same vectors"""
    import torch
    import bench
    g = golden("msm_r3.json")
    n = 1 << 20
    h = gpu.srs_generate(limbs(g["srs_secret_mont"]), n)
    for kind in bench.SKEWED_KINDS:
        case = g["skewed_2e20"][kind]
        sc = bench.skewed_scalars(kind, n)
        assert sha(sc) == case["scalars_sha256"], kind
        d = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
        _check(gpu.msm_device(h, d.data_ptr(), n), case)
        _check(gpu.msm_device(h, d.data_ptr(), 1 << 14), case["first_16384"])
        # three in flight: the MSMs behind the first take the throughput choices (two-step row / column sums, longer chunks) on the same heavy buckets
        tickets = [gpu.msm_device_async(h, d.data_ptr(), n) for _ in range(3)]
        for t in tickets:
            _check(gpu.msm_wait(t), case)
    gpu.srs_release(h)


def test_msm_plain_point_table(gpu, oracle, msm_small, golden):
    """bbgpu_msm_g1_plain = the reference's pippenger_low_memory convention (scalar_multiplication.cpp:142-262, test_scalar_multiplication.cpp:164-187):
    a PLAIN n-entry table of exactly n * 64 bytes.  The table ends right at the end of its buffer; result = the reference's own
    pippenger_low_memory output on the same inputs (= pippenger on the endomorphism table)"""
    g, srs, table, scalars = msm_small
    case = golden("msm_r3.json")["low_memory_1000"]
    n = case["n"]
    plain = aligned_copy(srs[:n])
    assert plain.nbytes == n * 64
    keep = scalars[:n].copy()
    _check(gpu.pippenger_low_memory(scalars, plain, n), case)
    assert np.array_equal(scalars[:n], keep)  # the reference may clobber its scalars; this entry does not
    for m in (1, 7, 24, 25, 999):
        want = oracle.msm_affine(scalars, table, m)
        assert np.array_equal(gpu.pippenger_low_memory(scalars, plain, m)[:8], want[:8]), m
    live0, auto0, _ = gpu.srs_cache_stats()
    gpu.pippenger_low_memory(scalars, plain, n)
    assert gpu.srs_cache_stats()[:2] == (live0, auto0)  # used once, never cached


def test_msm_row_range_shares_add_up(gpu, oracle, msm_small):
    """bbgpu_msm_g1_device_rows_async: shares of the W * n (window, point) pairs that start and end INSIDE digit windows (what bench.py
    gives N ranks when N does not divide W) add up to the MSM for N = 2, 3, 7, 8 and for ragged cuts; refused without window tables"""
    import torch
    from barretenberg_amd import BbGpuError
    g, srs, table, scalars = msm_small
    n = 1 << 14
    h = gpu.srs_register(table)
    d = torch.from_numpy(scalars[:n].view(np.int64)).cuda()
    if not gpu.srs_has_window_tables(h):
        with pytest.raises(BbGpuError):
            gpu.msm_device_rows_async(h, d.data_ptr(), n, 0, n)
        return
    want = oracle.msm_affine(scalars, table, n)
    W = gpu.srs_num_windows(h, n)
    R = W * n
    for cuts in ([0, R // 2, R], [0, R // 3, 2 * R // 3, R], [R * r // 7 for r in range(8)], [R * r // 8 for r in range(9)],
                 [0, 1, n - 1, n, n + 1, 5 * n + 17, R - 1, R]):
        parts = [gpu.msm_wait(gpu.msm_device_rows_async(h, d.data_ptr(), n, a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
        total = gpu.g1_sum(np.stack(parts))
        assert np.array_equal(total[:8], want[:8]), cuts
    with pytest.raises(BbGpuError):
        gpu.msm_device_rows_async(h, d.data_ptr(), n, 5, 5)
    with pytest.raises(BbGpuError):
        gpu.msm_device_rows_async(h, d.data_ptr(), n, 0, R + 1)


# ------------------------------------------------------------------ config 5: the reference prover on the GPU ----------
@pytest.mark.parametrize("build", ["plonk_gpu", "plonk_gpu_full"])
@pytest.mark.parametrize("gates", [32, 1024, 16384, 65536])
def test_reference_prover_runs_on_gpu_bit_exact(golden, gates, build):
    """BASELINE config 5.  oracle/_ref/plonk_gpu is the reference's UNMODIFIED StandardComposer -> waffle::Prover -> Verifier,
    compiled in the build container from the reference sources where they lie, with pippenger / batched_scalar_multiplications /
    the fft family resolved by barretenberg_amd/libbbshim.so -> libbbgpu.so (the INTEGRATION.md link recipe).  Its proof must be
    byte-identical to the one the all-CPU reference build produced for the same circuit and SRS, and must verify.
    `plonk_gpu_full` goes further: scalar_multiplication.o and polynomial_arithmetic.o are left out of the link altogether and the shim
    supplies every function the PLONK stack needs from them (evaluate, compute_kate_opening_coefficients, compute_lagrange_polynomial_fft,
    divide_by_pseudo_vanishing_polynomial, get_lagrange_evaluations, generate_pippenger_point_table besides the nine hot-path entries)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", build)
    srs = os.path.join(root, "oracle", "_ref", "transcript.dat")
    if not (os.path.exists(exe) and os.path.exists(srs)):
        pytest.fail("oracle/_ref/%s or its transcript is missing: the config-5 checker must travel with the repo (built by __graft_entry__.build() in the build container); a -m gpu run without it has lost its strongest parity evidence" % build)
    env = dict(os.environ, OMP_NUM_THREADS="16", BBGPU_SHIM_STRICT="1")  # the prover's own CPU loops: do not spawn one thread per host core of the box
    r = subprocess.run([exe, "prove", str(gates)], cwd=root, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.strip().split("\n")
    want = golden("plonk_proofs.json")["proofs"][str(gates)]
    assert got == want
    assert got[-1] == "verified 1"


@pytest.mark.parametrize("kind,gates", [("bool", 4096), ("mimc", 4094), ("extended", 160)])
def test_reference_prover_other_composers_on_gpu_bit_exact(golden, kind, gates):
    """the same link (plonk_gpu_full: every hot-path function from the shim) for the reference's BoolComposer, MiMCComposer and
    ExtendedComposer circuits -- their widgets call the same fft / coset_fft / batched_scalar_multiplications entry points
    (bool_widget.cpp:64-74,118-152, mimc_widget.cpp:60-67,125-160, sequential_widget.cpp:49-54,79-106): proofs byte-identical to the
    all-CPU build's, and verified by the reference Verifier"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "plonk_gpu_full")
    srs = os.path.join(root, "oracle", "_ref", "transcript.dat")
    if not (os.path.exists(exe) and os.path.exists(srs)):
        pytest.fail("oracle/_ref/plonk_gpu_full or its transcript is missing: the config-5 checker must travel with the repo (built by __graft_entry__.build() in the build container); a -m gpu run without it has lost its strongest parity evidence")
    env = dict(os.environ, OMP_NUM_THREADS="16", BB_CIRCUIT=kind, BBGPU_SHIM_STRICT="1")
    r = subprocess.run([exe, "prove", str(gates)], cwd=root, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.strip().split("\n")
    assert got == golden("plonk_trace.json")[kind]["proofs"][str(gates)]
    assert got[-1] == "verified 1"


@pytest.mark.parametrize("kind,gates", [("standard", 65536), ("bool", 4096), ("mimc", 4094), ("extended", 160)])
def test_reference_composer_to_resident_prover_adapter(golden, kind, gates):
    """INTEGRATION.md level 2, executable (oracle/plonk_driver.cpp `adapter`): the reference's own composer builds the circuit, the Prover
    state it assembles goes to bbgpu_plonk_prover_create unchanged (C++, the maintainer-side binding), the proof comes back in
    waffle::plonk_proof's layout, equals the all-CPU reference prover's byte for byte, and the reference Verifier accepts it"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "plonk_gpu")
    srs = os.path.join(root, "oracle", "_ref", "transcript.dat")
    if not (os.path.exists(exe) and os.path.exists(srs)):
        pytest.fail("oracle/_ref/plonk_gpu or its transcript is missing: the config-5 checker must travel with the repo (built by __graft_entry__.build() in the build container); a -m gpu run without it has lost its strongest parity evidence")
    env = dict(os.environ, OMP_NUM_THREADS="16", BBGPU_SHIM_STRICT="1")
    if kind != "standard":
        env["BB_CIRCUIT"] = kind
    r = subprocess.run([exe, "adapter", str(gates)], cwd=root, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    got = r.stdout.strip().split("\n")
    want = golden("plonk_proofs.json")["proofs"][str(gates)] if kind == "standard" else golden("plonk_trace.json")[kind]["proofs"][str(gates)]
    assert got == want
