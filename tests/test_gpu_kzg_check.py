"""bbgpu_kzg_check_openings / bbgpu_kzg_check_open_all on the GPU (-m gpu): the kernels of csrc/kzg_check.hip (k_kzg_claims in its three
instantiations, k_kzg_fold, k_kzg_fold_finish) and the driver in capi.hip against the host twins (csrc/host_kzg_check_batch.hpp), report against report,
field for field, a and b included, under a fixed seed -- the twins themselves are held to the 64-claim check the library had before by
tests/test_kzg_check_host.py.  Counts: 1 (the smallest call), 63 / 64 / 65 (the wave edge), 255 / 256 / 257 (the workgroup edge), 1023 / 1025 (the
small-table threshold of the transient MSM), 20480 (proofs across two 1 MiB upload chunks, a fold of more than one range).  The open-all form takes
count = batch x 2^k with batch <= 64 only: of the counts above that is 1, 63, 64 and 256; 65, 255, 257, 1023 and 1025 have no such factorisation (they
are covered there by (2, 1), (64, 3), (256, 16) and (4096, 5)).  Past the grid of k_kzg_claims (2048 workgroups of 256, so claim 2^19 is the first that
a thread takes in its second trip): 2^19 + 257 claims in the shared and the per-claim form, 33 x 2^14 (a partial second trip) and 64 x 2^14 (two full
trips, all 256 fold ranges) in the open-all form, over one world of 2^20 claims that the device producers make once."""
import time

import numpy as np
import pytest

from oracle.pyoracle import aligned_copy
from tests.kzg_check_cases import SEED, claims_of, expanded, honest, make_world, negated, off_curve, plus_one, scalars, secret_x
from tests.kzg_open_all_cases import INF

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
HALF = 1 << 19  # the threads of the k_kzg_claims grid at its cap: claim HALF + i is thread i's second
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1023, 1025]
POSITIONS = [0, 63, 64, 256, 299]  # of 300 claims: the first, both sides of the wave edge, the first of the second workgroup, the last
# the funnels one warm call of 256 claims passes (include/bbgpu.h).  Uploads: the proofs, y, z, then the commitments (per-claim layout) or the labels
# (shared layout), then the head (the findings' start value, the shared rows, G); the open-all form has neither z nor labels.  One read-back: the
# findings.  Launch checks: k_kzg_claims, k_kzg_fold, and one per MSM ticket.  No allocation: the staging buffer and the MSM workspaces are kept.
WARM = {"per_claim": dict(alloc_calls=0, h2d_calls=5, d2h_calls=1, launch_checks=4), "shared": dict(alloc_calls=0, h2d_calls=5, d2h_calls=1, launch_checks=4),
        "open_all": dict(alloc_calls=0, h2d_calls=3, d2h_calls=1, launch_checks=4)}
# with a finding: no fold and no ticket
WARM_FINDING = dict(alloc_calls=0, h2d_calls=5, d2h_calls=1, launch_checks=1)


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def W(lib, oracle, tmp_path_factory):
    """256 x 5 = 1280 true claims at domain points (every fifth of them with its proof at infinity); the claims of a test are drawn from it"""
    return make_world(lib, oracle, tmp_path_factory.mktemp("kzg_check"), 256, 5)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def device_world(lib, oracle, W, n, batch):
    """batch polynomials of n coefficients committed to, evaluated and opened at every domain point BY THE DEVICE (bbgpu_msm_g1_device,
    bbgpu_ntt_device_batch, bbgpu_kzg_open_all_device): commitments (batch, 8), values (batch, n, 4), proofs (batch, n, 8)"""
    import torch
    h = lib.srs_generate(secret_x(oracle), n)
    try:
        c = aligned_copy(oracle.random_scalars(0xD0A + n, batch * n))
        d_c = dev(c)
        setup = lib.kzg_open_all_setup(h, n)
        try:
            proofs = lib.kzg_open_all_device(setup, d_c.data_ptr(), n, batch=batch)
        finally:
            lib.kzg_open_all_release(setup)
        d_y = d_c.clone()
        torch.cuda.synchronize()
        commitments = np.stack([lib.msm_device(h, d_c.data_ptr() + b * n * 32, n)[:8] for b in range(batch)])
        lib.ntt_device_batch(d_y.data_ptr(), n, batch, "fft")
        torch.cuda.synchronize()
        return dict(n=n, batch=batch, g2_x=W["g2_x"], commitments=commitments, values=d_y.cpu().numpy().view(np.uint64).reshape(batch, n, 4), proofs=proofs)
    finally:
        lib.srs_release(h)


def both(lib, W, form, which, z, y, p, commitments=None, **kw):
    """(device report, twin report) of one call in the per-claim or the shared layout"""
    if form == "per_claim":
        args = (expanded(W, which) if commitments is None else commitments, z, y, p, W["g2_x"])
    else:
        args, kw = (W["commitments"] if commitments is None else commitments, z, y, p, W["g2_x"]), dict(kw, which=which)
    return lib.kzg_check_openings(*args, seed=SEED, **kw), lib.host_kzg_check_openings_batch(*args, seed=SEED, **kw)


def both_open_all(lib, V, values=None, proofs=None, commitments=None, stride=None, **kw):
    args = (V["commitments"] if commitments is None else commitments, V["values"] if values is None else values, V["proofs"] if proofs is None else proofs,
            V["n"], V["g2_x"])
    return lib.kzg_check_open_all(*args, stride=stride, seed=SEED, **kw), lib.host_kzg_check_open_all(*args, stride=stride, seed=SEED, **kw)


def wrong_proof(oracle, W, p):
    return W["table"][0].copy() if np.array_equal(p, INF) else negated(oracle, p)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("form", ["per_claim", "shared"])
def test_device_against_twin(lib, oracle, W, form, count):
    """true claims, and the same with one false value located: the whole report"""
    which, z, y, p = claims_of(W, count, start=count)
    got, want = both(lib, W, form, which, z, y, p)
    assert got == want and scalars(got) == honest(count)
    y2 = y.copy()
    y2[count // 2] = plus_one(oracle, y[count // 2])
    got, want = both(lib, W, form, which, z, y2, p, locate=True)
    assert got == want and got["ok"] == 0 and got["first_failing"] == count // 2
    assert lib.fault_stats()["slots_pending"] == 0


@pytest.mark.parametrize("n,batch,pad", [(1, 1, 0), (1, 63, 0), (1, 64, 3), (64, 1, 0), (256, 1, 0), (2, 1, 0), (64, 3, 5)])
def test_open_all_form_against_twin(lib, oracle, W, tmp_path, n, batch, pad):
    """the counts 1, 63, 64 and 256 as batch x n, then (2, 1) and (64, 3); with padding between the polynomials' values"""
    V = make_world(lib, oracle, tmp_path, n, batch)
    stride = n + pad
    values = aligned_copy(oracle.random_scalars(0x57D + n, batch * stride))
    for b in range(batch):
        values[b * stride:b * stride + n] = V["values"][b]
    got, want = both_open_all(lib, V, values=values, stride=stride)
    assert got == want and scalars(got) == honest(n * batch)
    values[(batch - 1) * stride + n - 1] = plus_one(oracle, values[(batch - 1) * stride + n - 1])
    got, want = both_open_all(lib, V, values=values, stride=stride, locate=True)
    assert got == want and got["ok"] == 0 and got["first_failing"] == n * batch - 1


def test_open_all_256_by_16(lib, oracle, W):
    """4096 claims over 16 commitments: the labels t >> 8 of the fold; a false value in polynomial 9"""
    V = device_world(lib, oracle, W, 256, 16)
    got, want = both_open_all(lib, V)
    assert got == want and scalars(got) == honest(4096)
    values = V["values"].copy()
    values[9, 17] = plus_one(oracle, values[9, 17])
    got, want = both_open_all(lib, V, values=values, locate=True)
    assert got == want and got["first_failing"] == 9 * 256 + 17


def test_the_proofs_of_open_all_device_are_accepted(lib, oracle, W):
    """(n, batch) = (4096, 5), 20,480 claims: what bbgpu_kzg_open_all_device wrote is checked in one call and the call says ok; the proofs cross two
    upload chunks and the fold takes five ranges and the finish kernel.  The same claims in the shared layout with explicit z (labels from memory)."""
    from tests.kzg_open_all_cases import domain
    n, batch = 4096, 5
    V = device_world(lib, oracle, W, n, batch)
    got, want = both_open_all(lib, V)
    print("timing of the call at 20480 claims:", lib.kzg_check_last_timing())
    assert got["ok"] == 1 and got == want and scalars(got) == honest(n * batch)
    t = np.arange(n * batch)
    explicit = lib.kzg_check_openings(V["commitments"], aligned_copy(domain(oracle, n)[t % n]), aligned_copy(V["values"].reshape(-1, 4)),
                                      aligned_copy(V["proofs"].reshape(-1, 8)), V["g2_x"], which=t // n, seed=SEED)
    assert explicit == got
    proofs = V["proofs"].copy()
    proofs[4, n - 1] = negated(oracle, proofs[4, n - 1])
    got, want = both_open_all(lib, V, proofs=proofs, locate=True)
    assert got == want and got["ok"] == 0 and got["first_failing"] == n * batch - 1 and got["rounds"] <= 1 + 15


@pytest.fixture(scope="module")
def big(lib, oracle, W):
    """(n, batch) = (2^14, 64) by the device producers: 2^20 true claims, every proof finite; z: the domain.  Made once, never written to."""
    from tests.kzg_open_all_cases import domain
    t0 = time.perf_counter()
    V = device_world(lib, oracle, W, 1 << 14, 64)
    print("producers of the world of 2^20 claims: %.2f s" % (time.perf_counter() - t0))
    return dict(V, z=domain(oracle, 1 << 14))


def first_polynomials(V, batch):
    return dict(V, batch=batch, commitments=V["commitments"][:batch], values=V["values"][:batch], proofs=V["proofs"][:batch])


def first_claims(V, count):
    """claims t < count of the world in the shared layout with explicit z: claim t is point t % n of polynomial t // n -> (which, z, y, proofs)"""
    t, n = np.arange(count), V["n"]
    return ((t // n).astype(np.uint32), aligned_copy(V["z"][t % n]), aligned_copy(V["values"].reshape(-1, 4)[:count]),
            aligned_copy(V["proofs"].reshape(-1, 8)[:count]))


def open_all_report(lib, V, values=None, proofs=None, **kw):
    return lib.kzg_check_open_all(V["commitments"], V["values"] if values is None else values, V["proofs"] if proofs is None else proofs, V["n"], V["g2_x"],
                                  seed=SEED, **kw)


@pytest.mark.parametrize("batch", [33, 64])
def test_open_all_form_past_the_claim_grid(lib, oracle, big, batch):
    """540,672 claims: threads 0 .. 16383 take two claims, the others one; 2^20 claims: two full trips and 256 fold ranges.  The call says ok; a false
    value at the last claim of the first trip, at the first of the second and at the last claim, and a negated proof inside the second trip's first
    workgroup, are each located exactly.  No twin at this size: the located claim is the reference."""
    V = first_polynomials(big, batch)
    n, count = V["n"], batch * V["n"]
    got = open_all_report(lib, V)
    assert got["ok"] == 1 and scalars(got) == honest(count)
    for t in (HALF - 1, HALF, count - 1):
        values = V["values"].copy()
        values[t // n, t % n] = plus_one(oracle, values[t // n, t % n])
        got = open_all_report(lib, V, values=values, locate=True)
        assert got["ok"] == 0 and got["first_failing"] == t and got["count"] == count, (t, got)
    t = HALF + 129
    proofs = V["proofs"].copy()
    proofs[t // n, t % n] = negated(oracle, proofs[t // n, t % n])
    got = open_all_report(lib, V, proofs=proofs, locate=True)
    assert got["ok"] == 0 and got["first_failing"] == t, got
    assert lib.fault_stats()["slots_pending"] == 0


def test_shared_and_per_claim_forms_past_the_claim_grid(lib, oracle, big):
    """2^19 + 257 claims over 33 commitments: 257 threads take a second claim.  Honest, and a false value at claim 2^19 + 100 located, in both forms; and
    at 33 x 2^14 claims the shared form with explicit z gives the open-all form's report, a and b included."""
    count, g2_x = HALF + 257, big["g2_x"]
    which, z, y, p = first_claims(big, count)
    cs = aligned_copy(big["commitments"][:33])
    Cs = aligned_copy(cs[which])
    assert int(which[-1]) == 32
    assert scalars(lib.kzg_check_openings(cs, z, y, p, g2_x, which=which, seed=SEED)) == honest(count)
    assert scalars(lib.kzg_check_openings(Cs, z, y, p, g2_x, seed=SEED)) == honest(count)
    y2 = y.copy()
    y2[HALF + 100] = plus_one(oracle, y[HALF + 100])
    for commitments, kw in ((cs, dict(which=which)), (Cs, {})):
        got = lib.kzg_check_openings(commitments, z, y2, p, g2_x, seed=SEED, locate=True, **kw)
        assert got["ok"] == 0 and got["first_failing"] == HALF + 100 and got["count"] == count, got
    V = first_polynomials(big, 33)
    which, z, y, p = first_claims(big, 33 * V["n"])
    assert lib.kzg_check_openings(cs, z, y, p, g2_x, which=which, seed=SEED) == open_all_report(lib, V)


def test_findings_of_the_second_trip(lib, oracle, big):
    """off-curve points at claims a thread meets in its second trip: the count and the first finding are exact (the key of a per-claim commitment is 2 t,
    of a proof 2 t + 1); with a finding in each trip of ONE thread (claims 5 and 2^19 + 5) the count is the sum and the first is the first trip's"""
    count, g2_x, t = HALF + 257, big["g2_x"], HALF + 5
    which, z, y, p = first_claims(big, count)
    cs = aligned_copy(big["commitments"][:33])
    Cs = aligned_copy(cs[which])
    V = first_polynomials(big, 33)
    n = V["n"]
    for spots in ((t,), (5, t)):
        p2, proofs = p.copy(), V["proofs"].copy()
        for s in spots:
            p2[s] = off_curve(oracle, p[s])
            proofs[s // n, s % n] = off_curve(oracle, proofs[s // n, s % n])
        found = dict(ok=0, rounds=0, bad_points=len(spots), first_bad=spots[0], first_bad_is_proof=1)
        assert scalars(lib.kzg_check_openings(cs, z, y, p2, g2_x, which=which, seed=SEED)) == honest(count, **found), spots
        assert scalars(lib.kzg_check_openings(Cs, z, y, p2, g2_x, seed=SEED)) == honest(count, **found), spots
        assert scalars(open_all_report(lib, V, proofs=proofs)) == honest(33 * n, **found), spots
    c2, p2 = Cs.copy(), p.copy()
    c2[t], p2[t - 1] = off_curve(oracle, Cs[t]), off_curve(oracle, p[t - 1])  # keys 2 t and 2 (t - 1) + 1: the proof comes first
    got = lib.kzg_check_openings(c2, z, y, p2, g2_x, seed=SEED)
    assert scalars(got) == honest(count, ok=0, rounds=0, bad_points=2, first_bad=t - 1, first_bad_is_proof=1)
    assert scalars(lib.kzg_check_openings(cs, z, y, p, g2_x, which=which, seed=SEED)) == honest(count)  # the next call is the honest one


def test_the_twin_past_the_claim_grid(lib, big):
    """the shared form at 2^19 + 257 claims, report against report; the twin's wall time is printed"""
    count = HALF + 257
    which, z, y, p = first_claims(big, count)
    cs = aligned_copy(big["commitments"][:33])
    got = lib.kzg_check_openings(cs, z, y, p, big["g2_x"], which=which, seed=SEED)
    t0 = time.perf_counter()
    want = lib.host_kzg_check_openings_batch(cs, z, y, p, big["g2_x"], which=which, seed=SEED)
    print("host twin at %d claims: %.2f s" % (count, time.perf_counter() - t0))
    assert got == want and got["ok"] == 1


@pytest.mark.parametrize("t", POSITIONS)
def test_tampered_claims_are_located(lib, oracle, W, t):
    """a value, a proof or a commitment changed at claim t of 300: ok = 0 and the bisection names t, in every form that has such an input"""
    count = 300
    which, z, y, p = claims_of(W, count)
    y2, p2, c2 = y.copy(), p.copy(), expanded(W, which)
    y2[t] = plus_one(oracle, y[t])
    p2[t] = wrong_proof(oracle, W, p[t])
    c2[t] = negated(oracle, c2[t])
    for form, args, kw in (("per_claim", (y2, p), {}), ("per_claim", (y, p2), {}), ("per_claim", (y, p), dict(commitments=c2)), ("shared", (y2, p), {}),
                           ("shared", (y, p2), {})):
        got, want = both(lib, W, form, which, z, *args, locate=True, **kw)
        assert got == want and got["ok"] == 0 and got["first_failing"] == t and 2 <= got["rounds"] <= 10, (form, got)
        assert both(lib, W, form, which, z, *args, **kw)[0]["first_failing"] == -1  # without the flag nothing is located
    # a shared commitment changed: the first claim that bears its label
    sh = W["commitments"].copy()
    sh[t % 5] = negated(oracle, sh[t % 5])
    got, want = both(lib, W, "shared", which, z, y, p, commitments=sh, locate=True)
    assert got == want and got["first_failing"] == int(np.argmax(which == t % 5))
    # the open-all form: 256 x 5 claims, the value of claim t
    values = W["values"].copy()
    values[t // 256, t % 256] = plus_one(oracle, values[t // 256, t % 256])
    got, want = both_open_all(lib, W, values=values, locate=True)
    assert got == want and got["first_failing"] == t


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_points_off_the_curve_are_findings(lib, oracle, W):
    """off-curve points in the first and in the last wave of 300 claims: the counts and the first finding are exact, and no fold and no ticket is issued
    (one launch check, k_kzg_claims')"""
    count = 300
    which, z, y, p = claims_of(W, count)
    Cs = expanded(W, which)
    first, last = 5, 299  # claims of polynomials 0 and 4: finite proofs
    for spots in ((first,), (last,), (first, last)):
        p2 = p.copy()
        for t in spots:
            p2[t] = off_curve(oracle, p[t])
        for form in ("per_claim", "shared"):
            lib.kzg_check_openings(Cs, z, y, p2, W["g2_x"], seed=SEED)  # warm
            (got, want), st = counted(lib, lambda: both(lib, W, form, which, z, y, p2, locate=True), WARM_FINDING)
            assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=len(spots), first_bad=spots[0], first_bad_is_proof=1), (form, got)
            assert st == WARM_FINDING and lib.fault_stats()["slots_pending"] == 0, st
    c2, p2 = Cs.copy(), p.copy()
    c2[last], c2[first], p2[first] = off_curve(oracle, Cs[last]), off_curve(oracle, Cs[first]), off_curve(oracle, p[first])
    got, want = both(lib, W, "per_claim", which, z, y, p2, commitments=c2)
    assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=3, first_bad=first, first_bad_is_proof=0)
    c2[first] = Cs[first]
    got, want = both(lib, W, "per_claim", which, z, y, p2, commitments=c2)  # pi_5 now comes first
    assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=2, first_bad=first, first_bad_is_proof=1)
    sh = W["commitments"].copy()
    sh[3] = off_curve(oracle, sh[3])
    got, want = both(lib, W, "shared", which, z, y, p2, commitments=sh)  # a shared commitment comes before every claim
    assert got == want and scalars(got) == honest(count, ok=0, rounds=0, bad_points=2, first_bad=3, first_bad_is_proof=0)
    proofs = W["proofs"].copy()
    proofs[4, 255], proofs[0, 0] = off_curve(oracle, proofs[4, 255]), off_curve(oracle, proofs[0, 0])
    got, want = both_open_all(lib, W, proofs=proofs, commitments=sh)
    assert got == want and scalars(got) == honest(1280, ok=0, rounds=0, bad_points=3, first_bad=3, first_bad_is_proof=0)
    got, want = both_open_all(lib, W, proofs=proofs)
    assert got == want and scalars(got) == honest(1280, ok=0, rounds=0, bad_points=2, first_bad=0, first_bad_is_proof=1)
    got, want = both(lib, W, "shared", which, z, y, p)  # the next call is the honest one
    assert got == want and got["ok"] == 1


def test_infinities_duplicates_and_exchanged_labels(lib, oracle, W):
    n = 256
    # every proof at infinity (the constant polynomial): B is the point at infinity, in every form
    const = (np.ones(n, dtype=np.uint32), aligned_copy(W["z"]), aligned_copy(W["values"][1]), aligned_copy(W["proofs"][1]))
    for form in ("per_claim", "shared"):
        got, want = both(lib, W, form, *const)
        assert got == want and scalars(got) == honest(n) and got["b"] == [int(v) for v in INF]
    # a commitment at infinity with the claim 0 = 0 among others, shared and per claim
    which, z, y, p = claims_of(W, 70)
    sh = W["commitments"].copy()
    sh[1] = INF
    y0 = y.copy()
    y0[which == 1] = 0
    for form, cs in (("shared", sh), ("per_claim", aligned_copy(sh[which]))):
        got, want = both(lib, W, form, which, z, y0, p, commitments=cs)
        assert got == want and scalars(got) == honest(70)
    # duplicate claims: 200 copies of one claim between others -- colliding rows in both MSMs
    which, z, y, p = claims_of(W, 300)
    idx = np.concatenate([np.arange(50), np.full(200, 7), np.arange(50, 100)])
    dup = [aligned_copy(v[idx]) for v in (which, z, y, p)]
    for form in ("per_claim", "shared"):
        got, want = both(lib, W, form, *dup)
        assert got == want and scalars(got) == honest(300)
    y2 = dup[2].copy()
    y2[137] = plus_one(oracle, y2[137])  # one of the copies is false
    got, want = both(lib, W, "shared", dup[0], dup[1], y2, dup[3], locate=True)
    assert got == want and got["first_failing"] == 137
    # exchanged labels: claims 10 and 11 are of different polynomials
    swapped = which.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    assert which[10] != which[11]
    got, want = both(lib, W, "shared", swapped, z, y, p, locate=True)
    assert got == want and got["ok"] == 0 and got["first_failing"] == 10


def test_seed_rules_and_determinism(lib, W):
    which, z, y, p = claims_of(W, 100)
    runs = [lib.kzg_check_openings(W["commitments"], z, y, p, W["g2_x"], which=which, seed=SEED) for _ in range(2)]
    assert runs[0] == runs[1]
    drawn = [lib.kzg_check_openings(W["commitments"], z, y, p, W["g2_x"], which=which) for _ in range(2)]
    assert all(r["ok"] == 1 for r in drawn) and drawn[0]["seed"] != drawn[1]["seed"] and drawn[0]["a"] != drawn[1]["a"]
    replay = lib.host_kzg_check_openings_batch(W["commitments"], z, y, p, W["g2_x"], which=which, seed=np.array(drawn[0]["seed"], dtype=np.uint64))
    assert replay == drawn[0]


def calls(lib, W):
    which, z, y, p = claims_of(W, 256)
    V = dict(W, commitments=W["commitments"][:1], values=W["values"][:1], proofs=W["proofs"][:1])
    return {"per_claim": lambda **kw: both(lib, W, "per_claim", which, z, y, p, **kw), "shared": lambda **kw: both(lib, W, "shared", which, z, y, p, **kw),
            "open_all": lambda **kw: both_open_all(lib, V, **kw)}


def test_funnel_counts_of_warm_calls(lib, W):
    """256 claims in each form: the counts of include/bbgpu.h; the staging is counted in bbgpu_memory_stats"""
    for form, run in calls(lib, W).items():
        run()  # warm
        (got, want), st = counted(lib, run, WARM[form])  # the twin makes no HIP call: the counts are the device call's
        print("funnels of one warm call of 256 claims,", form, st)
        assert got["ok"] == 1 and st == WARM[form], (form, st)
    assert lib.memory_stats()["staging_bytes"] >= 256 * 480


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", ["per_claim", "shared", "open_all"])
def test_injected_failures_leave_nothing_behind(lib, oracle, W, form, kind):
    """every site of the funnel `kind` that one warm call with LOCATE over a false claim passes (fold and MSM rounds included), failed once.  These are
    the library's injected error returns; nothing faults on the device.  Each failure is an error return with no MSM slot pending and the live
    allocations of before, and the very next call gives the honest report."""
    from barretenberg_amd import BbGpuError
    which, z, y, p = claims_of(W, 256)
    y2 = y.copy()
    y2[200] = plus_one(oracle, y[200])
    values = W["values"][:1].copy()
    values[0, 200] = plus_one(oracle, values[0, 200])
    V = dict(W, commitments=W["commitments"][:1], values=values, proofs=W["proofs"][:1])
    if form == "open_all":
        run = lambda: lib.kzg_check_open_all(V["commitments"], V["values"], V["proofs"], 256, V["g2_x"], seed=SEED, locate=True)  # noqa: E731
        want = lib.host_kzg_check_open_all(V["commitments"], V["values"], V["proofs"], 256, V["g2_x"], seed=SEED, locate=True)
    else:
        run = lambda: both(lib, W, form, which, z, y2, p, locate=True)[0]  # noqa: E731
        want = both(lib, W, form, which, z, y2, p, locate=True)[1]
    assert run() == want and want["first_failing"] == 200  # warm
    lib.fault_inject("%s:%d" % (kind, FAR))
    assert run() == want
    st = lib.fault_stats()
    sites, live = st[KEYS[kind]], st["live_allocations"]
    assert sites >= WARM[form][KEYS[kind]], st
    for k in range(sites):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError, match=" -1:"):
            run()
        st = lib.fault_stats()
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["slots_pending"] == 0 and st["live_allocations"] == live, (kind, k, st)
        assert run() == want, (kind, k)
    lib.fault_inject(None)


def test_the_stage_timing_of_the_last_call(lib, W):
    """bbgpu_kzg_check_last_timing (diagnostic): non-negative wall times that add up to the total"""
    which, z, y, p = claims_of(W, 256)
    assert lib.kzg_check_openings(W["commitments"], z, y, p, W["g2_x"], which=which, seed=SEED)["ok"] == 1
    ms = lib.kzg_check_last_timing()
    assert all(v >= 0 for v in ms.values()) and ms["total_ms"] > 0 and ms["msm_ms"] > 0 and ms["host_tail_ms"] > 0
    assert abs(ms["total_ms"] - sum(v for k, v in ms.items() if k != "total_ms")) < 1e-6
