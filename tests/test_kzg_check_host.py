"""bbgpu_host_kzg_check_openings_batch / bbgpu_host_kzg_check_open_all (csrc/host_kzg_check_batch.hpp): the definition the GPU entries are compared with
field for field (tests/test_gpu_kzg_check.py), against the check the library had before (bbgpu_host_kzg_check_openings, 64 claims), the three forms against
each other, the named cases, the bisection, and the argument verdicts of all four entries on a machine without a GPU.  CPU tests; the claims are
tests/kzg_check_cases.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import aligned_copy, from_int
from tests.kzg_check_cases import (ERR_ARG, ERR_SIZE, NONE, SEED, above_r, claims_of, expanded, honest, make_world, negated, off_curve, off_domain_claim,
                                   plus_one, scalars)
from tests.kzg_open_all_cases import INF

N, BATCH = 16, 3


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def W(lib, oracle, tmp_path_factory):
    return make_world(lib, oracle, tmp_path_factory.mktemp("kzg_check"), N, BATCH)


def per_claim(lib, W, which, z, y, p, **kw):
    return lib.host_kzg_check_openings_batch(expanded(W, which), z, y, p, W["g2_x"], **kw)


def shared(lib, W, which, z, y, p, **kw):
    return lib.host_kzg_check_openings_batch(W["commitments"], z, y, p, W["g2_x"], which=which, **kw)


def wrong_proof(oracle, W, p):
    """another point on the curve in place of a proof: the negated proof, or the generator for a proof at infinity"""
    return W["table"][0].copy() if np.array_equal(p, INF) else negated(oracle, p)


@pytest.mark.parametrize("count", [1, 2, 33, 48])
def test_against_the_existing_check(lib, oracle, W, count):
    """count <= 64, per-claim layout, the same seed: the verdict of bbgpu_host_kzg_check_openings, honest and tampered (a value, a proof, a commitment)"""
    which, z, y, p = claims_of(W, count)
    Cs = expanded(W, which)
    old = lambda c, yy, pp: lib.host_kzg_check_openings(c, z, yy, pp, W["g2_x"], seed=SEED)  # noqa: E731
    new = lambda c, yy, pp: lib.host_kzg_check_openings_batch(c, z, yy, pp, W["g2_x"], seed=SEED)  # noqa: E731
    rep = new(Cs, y, p)
    assert old(Cs, y, p) is True and scalars(rep) == honest(count) and rep["seed"] == [int(v) for v in SEED]
    for t in sorted({0, count // 2, count - 1}):
        y2, p2, c2 = y.copy(), p.copy(), Cs.copy()
        y2[t] = plus_one(oracle, y[t])
        p2[t] = wrong_proof(oracle, W, p[t])
        c2[t] = negated(oracle, Cs[t])
        for args in ((Cs, y2, p), (Cs, y, p2), (c2, y, p)):
            assert old(*args) is False and scalars(new(*args)) == honest(count, ok=0), t


def test_a_seed_from_the_operating_system_is_reported(lib, W):
    which, z, y, p = claims_of(W, 5)
    a, b = per_claim(lib, W, which, z, y, p), per_claim(lib, W, which, z, y, p)
    assert a["ok"] == b["ok"] == 1 and a["seed"] != b["seed"] and a["a"] != b["a"]
    assert per_claim(lib, W, which, z, y, p, seed=np.array(a["seed"], dtype=np.uint64)) == a  # a finding can be replayed


@pytest.mark.parametrize("count", [1, 7, 48])
def test_shared_layout_against_per_claim_layout(lib, oracle, W, count):
    """the same claims with shared commitments and expanded: the same report, a and b included; also when a claim is false"""
    which, z, y, p = claims_of(W, count)
    assert shared(lib, W, which, z, y, p, seed=SEED) == per_claim(lib, W, which, z, y, p, seed=SEED)
    y2 = y.copy()
    y2[count // 2] = plus_one(oracle, y[count // 2])
    got = shared(lib, W, which, z, y2, p, seed=SEED, locate=True)
    assert got == per_claim(lib, W, which, z, y2, p, seed=SEED, locate=True) and got["ok"] == 0 and got["first_failing"] == count // 2


@pytest.mark.parametrize("n,batch,pad", [(1, 1, 0), (2, 1, 0), (4, 3, 5), (N, BATCH, 0), (N, BATCH, 5)])
def test_open_all_form_against_the_shared_layout(lib, oracle, W, tmp_path, n, batch, pad):
    """the report of the shared layout with explicit z = omega^i and labels b, a and b included; the values may be padded"""
    V = W if n == N else make_world(lib, oracle, tmp_path, n, batch)
    stride = n + pad
    values = aligned_copy(oracle.random_scalars(0x57D + n, batch * stride))
    for b in range(batch):
        values[b * stride:b * stride + n] = V["values"][b]
    t = np.arange(n * batch)
    want = lib.host_kzg_check_openings_batch(V["commitments"], aligned_copy(V["z"][t % n]), aligned_copy(V["values"].reshape(-1, 4)),
                                             aligned_copy(V["proofs"].reshape(-1, 8)), V["g2_x"], which=t // n, seed=SEED)
    got = lib.host_kzg_check_open_all(V["commitments"], values, V["proofs"], n, V["g2_x"], stride=stride, seed=SEED)
    assert got == want and scalars(got) == honest(n * batch)
    bad = values.copy()
    bad[(batch - 1) * stride + n - 1] = plus_one(oracle, bad[(batch - 1) * stride + n - 1])
    got = lib.host_kzg_check_open_all(V["commitments"], bad, V["proofs"], n, V["g2_x"], stride=stride, seed=SEED, locate=True)
    assert got["ok"] == 0 and got["first_failing"] == n * batch - 1
    if pad:  # the padding is not read
        other = values.copy()
        other[n:stride] = plus_one(oracle, other[n])
        assert lib.host_kzg_check_open_all(V["commitments"], other, V["proofs"], n, V["g2_x"], stride=stride, seed=SEED) == want


def test_named_cases(lib, oracle, W):
    n = N
    # a constant polynomial: every proof is at infinity, B is the point at infinity
    const = (np.ones(n, dtype=np.uint32), aligned_copy(W["z"]), aligned_copy(W["values"][1]), aligned_copy(W["proofs"][1]))
    assert np.array_equal(const[3], np.tile(INF, (n, 1)))
    rep = shared(lib, W, *const, seed=SEED)
    assert scalars(rep) == honest(n) and rep["b"] == [int(v) for v in INF] and rep == per_claim(lib, W, *const, seed=SEED)
    other = const[2].copy()
    other[4] = plus_one(oracle, other[4])
    assert shared(lib, W, const[0], const[1], other, const[3], seed=SEED)["ok"] == 0
    # a commitment at infinity (the zero polynomial) with the claim 0 = 0, per claim and shared
    zero = dict(commitments=np.stack([W["commitments"][0], INF]), g2_x=W["g2_x"])
    which, z, y, p = np.array([0, 1, 1], dtype=np.uint32), aligned_copy(W["z"][[3, 5, 6]]), aligned_copy(np.stack([W["values"][0, 3], from_int(0), from_int(0)])), \
        aligned_copy(np.stack([W["proofs"][0, 3], INF, INF]))
    a, b = shared(lib, zero, which, z, y, p, seed=SEED), per_claim(lib, zero, which, z, y, p, seed=SEED)
    assert a == b and scalars(a) == honest(3)
    y[2] = plus_one(oracle, y[2])
    assert shared(lib, zero, which, z, y, p, seed=SEED)["ok"] == 0 and per_claim(lib, zero, which, z, y, p, seed=SEED)["ok"] == 0
    # the same claim twice
    which, z, y, p = claims_of(W, 4)
    twice = [aligned_copy(np.concatenate([v, v[2:3], v[2:3]])) for v in (which, z, y, p)]
    assert scalars(shared(lib, W, *twice, seed=SEED)) == honest(6) and scalars(per_claim(lib, W, *twice, seed=SEED)) == honest(6)
    # z on and off the domain, in one call
    offs = [off_domain_claim(lib, oracle, W, b, b) for b in (0, 2)]
    mixed = (np.array([0, 2, 0, 2], dtype=np.uint32), aligned_copy(np.stack([offs[0][0], offs[1][0], W["z"][5], W["z"][n - 1]])),
             aligned_copy(np.stack([offs[0][1], offs[1][1], W["values"][0, 5], W["values"][2, n - 1]])),
             aligned_copy(np.stack([offs[0][2], offs[1][2], W["proofs"][0, 5], W["proofs"][2, n - 1]])))
    want = shared(lib, W, *mixed, seed=SEED)
    assert scalars(want) == honest(4) and want == per_claim(lib, W, *mixed, seed=SEED)
    # a z and a y given as the representative in [r, 2r): the same report
    z2, y2 = mixed[1].copy(), mixed[2].copy()
    z2[0], y2[1], z2[2], y2[2] = above_r(z2[0]), above_r(y2[1]), above_r(z2[2]), above_r(y2[2])
    assert shared(lib, W, mixed[0], z2, y2, mixed[3], seed=SEED) == want and per_claim(lib, W, mixed[0], z2, y2, mixed[3], seed=SEED) == want
    # a proof under the wrong label fails the pairing
    swapped = mixed[0].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert scalars(shared(lib, W, swapped, *mixed[1:], seed=SEED, locate=True)) == honest(4, ok=0, rounds=3, first_failing=0)


def test_points_off_the_curve_are_findings(lib, oracle, W):
    """a finite point off the curve is counted and named, ok = 0, no sums are taken (a and b stay at infinity); the existing entry refuses the same input"""
    from barretenberg_amd import BbGpuError
    which, z, y, p = claims_of(W, 9)
    Cs = expanded(W, which)
    inf = [int(v) for v in INF]
    p2 = p.copy()
    p2[3], p2[6] = off_curve(oracle, p[3]), off_curve(oracle, p[6])  # claims 3 and 6 have finite proofs (polynomials 0)
    for rep in (per_claim(lib, W, which, z, y, p2, seed=SEED, locate=True), shared(lib, W, which, z, y, p2, seed=SEED, locate=True)):
        assert scalars(rep) == honest(9, ok=0, rounds=0, bad_points=2, first_bad=3, first_bad_is_proof=1) and rep["a"] == inf and rep["b"] == inf
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.host_kzg_check_openings(Cs, z, y, p2, W["g2_x"], seed=SEED)
    c2 = Cs.copy()
    c2[3], c2[8] = off_curve(oracle, Cs[3]), off_curve(oracle, Cs[8])
    rep = lib.host_kzg_check_openings_batch(c2, z, y, p2, W["g2_x"], seed=SEED)  # C_3 comes before pi_3
    assert scalars(rep) == honest(9, ok=0, rounds=0, bad_points=4, first_bad=3, first_bad_is_proof=0)
    sh = W["commitments"].copy()
    sh[2] = off_curve(oracle, sh[2])
    rep = lib.host_kzg_check_openings_batch(sh, z, y, p2, W["g2_x"], which=which, seed=SEED)  # a shared commitment comes before every claim
    assert scalars(rep) == honest(9, ok=0, rounds=0, bad_points=3, first_bad=2, first_bad_is_proof=0)
    rep = lib.host_kzg_check_open_all(sh, W["values"], W["proofs"], N, W["g2_x"], seed=SEED)
    assert scalars(rep) == honest(N * BATCH, ok=0, rounds=0, bad_points=1, first_bad=2, first_bad_is_proof=0)
    pr = W["proofs"].copy()
    pr[2, N - 1] = off_curve(oracle, pr[2, N - 1])
    rep = lib.host_kzg_check_open_all(W["commitments"], W["values"], pr, N, W["g2_x"], seed=SEED)
    assert scalars(rep) == honest(N * BATCH, ok=0, rounds=0, bad_points=1, first_bad=N * BATCH - 1, first_bad_is_proof=1)


@pytest.mark.parametrize("count", [1, 2, 47])
def test_locate(lib, oracle, W, count):
    """a tampered y or pi at position 0, middle and last is located, in at most ceil(log2 count) more rounds; two false claims: the first"""
    which, z, y, p = claims_of(W, count)
    for t in sorted({0, count // 2, count - 1}):
        y2, p2 = y.copy(), p.copy()
        y2[t] = plus_one(oracle, y[t])
        p2[t] = wrong_proof(oracle, W, p[t])
        for args in ((y2, p), (y, p2)):
            for form in (per_claim, shared):
                rep = form(lib, W, which, z, *args, seed=SEED, locate=True)
                assert rep["ok"] == 0 and rep["first_failing"] == t and 1 <= rep["rounds"] <= 1 + max(count - 1, 0).bit_length(), (t, rep)
                assert scalars(form(lib, W, which, z, *args, seed=SEED)) == honest(count, ok=0)  # without the flag: one round, nothing located
    if count > 2:
        y2 = y.copy()
        y2[3], y2[count - 2] = plus_one(oracle, y[3]), plus_one(oracle, y[count - 2])
        assert shared(lib, W, which, z, y2, p, seed=SEED, locate=True)["first_failing"] == 3
    assert scalars(shared(lib, W, which, z, y, p, seed=SEED, locate=True)) == honest(count)  # nothing to locate


def test_argument_errors(lib, oracle, W):
    """every argument error of the four entries -- the device entries refuse before a device is bound, so a machine without a GPU gives the same verdicts"""
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import KzgCheckReport, _ptr, u64p
    which, z, y, p = claims_of(W, 6)
    Cs, g2 = expanded(W, which), W["g2_x"]
    u32p = C.POINTER(C.c_uint32)
    rep = KzgCheckReport()
    seed = aligned_copy(SEED)
    bad_g2 = g2.copy()
    bad_g2[0] ^= 1
    inf_g2 = g2.copy()
    inf_g2[15] |= np.uint64(1 << 63)
    labels = lambda w: np.ascontiguousarray(w, dtype=np.uint32).ctypes.data_as(u32p)  # noqa: E731
    for fn in (lib.lib.bbgpu_kzg_check_openings, lib.lib.bbgpu_host_kzg_check_openings_batch):
        fn.argtypes = [u64p, u32p, C.c_size_t, u64p, u64p, u64p, C.c_size_t, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        good = [_ptr(Cs), None, 0, _ptr(z), _ptr(y), _ptr(p), 6, _ptr(g2), _ptr(seed), 0, C.byref(rep)]
        good_shared = [_ptr(W["commitments"]), labels(which), BATCH] + good[3:]

        def refused(args, **changes):
            a = list(args)
            for k, v in changes.items():
                a[int(k[1:])] = v
            return fn(*a)

        for count in (0, (1 << 20) + 1):
            assert refused(good, a6=count) == -2 and refused(good_shared, a6=count) == -2
        for k in (0, 3, 4, 5, 7, 10):  # null commitments / z / y / proofs / g2_x / report
            assert refused(good, **{"a%d" % k: None}) == -3, k
            assert refused(good_shared, **{"a%d" % k: None}) == -3, k
        for flags in (2, 4, -1):
            assert refused(good, a9=flags) == -3
        for g in (bad_g2, inf_g2):
            assert refused(good, a7=_ptr(g)) == -3
        for num in (0, 65):
            assert refused(good_shared, a2=num) == -3
        assert refused(good_shared, a1=labels([0, 1, 2, 3, 0, 1])) == -3 and refused(good_shared, a2=2) == -3  # a label out of range
        if fn is lib.lib.bbgpu_host_kzg_check_openings_batch:  # the calls themselves are good (the device entry would go on to bind a device)
            assert refused(good, a2=99) == 0 and rep.ok == 1  # num_commitments is not read without labels
            assert refused(good_shared) == 0 and rep.ok == 1
    for fn in (lib.lib.bbgpu_kzg_check_open_all, lib.lib.bbgpu_host_kzg_check_open_all):
        fn.argtypes = [u64p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_int, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        vals, proofs = aligned_copy(W["values"].reshape(-1, 4)), aligned_copy(W["proofs"].reshape(-1, 8))
        good = [_ptr(W["commitments"]), _ptr(vals), N, _ptr(proofs), N, BATCH, _ptr(g2), _ptr(seed), 0, C.byref(rep)]

        def refused_oa(**changes):
            a = list(good)
            for k, v in changes.items():
                a[int(k[1:])] = v
            return fn(*a)

        for n in (0, 3, 12, (1 << 20) + 1, 1 << 21):
            assert refused_oa(a4=n, a2=max(n, N)) == -2, n
        for batch in (0, -1, 65):
            assert refused_oa(a5=batch) == -2, batch
        assert refused_oa(a2=N - 1) == -2  # stride < n
        assert refused_oa(a4=1 << 15, a2=1 << 15, a5=33) == -2 and refused_oa(a4=1 << 20, a2=1 << 20, a5=2) == -2  # batch x n above 2^20
        for k in (0, 1, 3, 6, 9):
            assert refused_oa(**{"a%d" % k: None}) == -3, k
        assert refused_oa(a8=2) == -3 and refused_oa(a6=_ptr(bad_g2)) == -3
    # through the binding: the message names the entry's family
    with pytest.raises(BbGpuError, match=ERR_SIZE + " KZG check"):
        lib.kzg_check_openings(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64),
                               np.zeros((0, 8), dtype=np.uint64), g2, seed=SEED)
    with pytest.raises(BbGpuError, match=ERR_ARG + " KZG check"):
        lib.kzg_check_open_all(W["commitments"], W["values"], W["proofs"], N, bad_g2, seed=SEED)
    assert lib.lib.bbgpu_kzg_check_last_timing(None) == -3
    assert NONE == KzgCheckReport.NONE


def test_the_existing_entry_keeps_its_limit(lib, W):
    from barretenberg_amd import BbGpuError
    k = 65
    with pytest.raises(BbGpuError, match=ERR_SIZE):
        lib.host_kzg_check_openings(np.zeros((k, 8), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64),
                                    np.zeros((k, 8), dtype=np.uint64), W["g2_x"], seed=SEED)


def test_host_twins_under_sanitizers(tmp_path):
    """tests/cpp/test_kzg_check_host.cpp: the twins as a stand-alone program (own main) built with -fsanitize=address,undefined: the three forms against
    each other and against the 64-claim check, infinities, findings and the bisection, over a string the program makes itself"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kzg_check_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_kzg_check_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
