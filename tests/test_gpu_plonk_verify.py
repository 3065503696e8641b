"""bbgpu_plonk_verify_batch on the GPU (-m gpu): the per-proof work in k_verify_terms, the shared terms summed by k_verify_fold, A and B as two device
MSM tickets over the rows the kernel wrote, the pairing tail on the host.  Every report is compared, field for field and with a and b, with
bbgpu_host_plonk_verify_batch on the same proofs; expected verdicts are the reference's (tests/golden/plonk_verify.json), never this code's own.
Counts 1, 2, 63, 64, 65, 255, 256, 257, 1000 at 32 gates: one thread per proof in workgroups of 64, the fold in workgroups of 256."""
import os
import subprocess

import numpy as np
import pytest

from tests.plonk_verify_cases import BAD_POINT, NONE, ROOT, SEED, fields, fixture, row, row_ids, whole

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
FAR = 1 << 62
# funnel passes of one warm call without LOCATE, whatever the count up to 1092 proofs (one staging chunk of 1 MiB): no allocation; two uploads (the
# proofs, the shared rows); one read-back (the statuses); four launch checks (k_verify_terms, k_verify_fold, one per device MSM)
WARM = dict(alloc_calls=0, h2d_calls=2, d2h_calls=1, launch_checks=4)
SECRET = 0x0123456789ABCDEF0F1E2D3C4B5A6978FEDCBA98765432100123456789ABCDEF  # the x of oracle/_ref/transcript.dat and of the golden proofs


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def verifiers(lib):
    """one handle per circuit of the fixture, made once"""
    g2_x, circuits, _ = fixture()
    hs = {key: lib.plonk_verifier_create(c["n"], c["widgets"], c["vk"], g2_x) for key, c in circuits.items()}
    yield hs
    for h in hs.values():
        lib.plonk_verifier_destroy(h)


def both(lib, verifiers, circuit, proofs, seed=SEED, locate=True):
    """the GPU report and the host report of one batch; they must agree in every field, status, a and b included"""
    g2_x, circuits, _ = fixture()
    c = circuits[circuit]
    gpu = lib.plonk_verify_batch(verifiers[circuit], proofs, seed, locate)
    host = lib.host_plonk_verify_batch(c["n"], c["widgets"], c["vk"], g2_x, proofs, seed, locate)
    assert whole(gpu) == whole(host), (fields(gpu), fields(host), list(gpu.status), list(host.status))
    return gpu


@pytest.fixture(scope="module")
def pool(lib):
    """honest proofs of the 32-gate bench circuit: the golden one and 15 of distinct witnesses from ONE call of the batch prover; made once"""
    from oracle.pyoracle import FR_MODULUS
    from barretenberg_amd.plonk import Prover, bench_circuit, to_montgomery_limbs
    hs = lib.srs_generate(to_montgomery_limbs([SECRET % FR_MODULUS])[0], 1024)
    states = [bench_circuit(32, 3 + 5 * k, 7 + 11 * k).preprocess() for k in range(15)]
    P = Prover(lib, states[0], hs)
    proofs = P.construct_proofs([(s["w_l"], s["w_r"], s["w_o"]) for s in states])
    P.destroy()
    lib.srs_release(hs)
    out = np.concatenate([row("standard/32", "none")["proof"][None, :], proofs])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("r", fixture()[2], ids=row_ids())
def test_every_fixture_row_equals_the_host_twin(lib, verifiers, r):
    rep = both(lib, verifiers, r["circuit"], r["proof"])
    assert int(rep.status[0]) == r["status"] and rep.ok == bool(r["verdict"]), (r["tamper"], fields(rep))
    assert lib.fault_stats()["slots_pending"] == 0


def test_proofs_of_other_witnesses_are_accepted(lib, verifiers, pool):
    """16 honest proofs, 15 of them of witnesses the fixture has never seen; the reference's Verifier accepts one of them too"""
    from barretenberg_amd.plonk import proof_lines
    rep = both(lib, verifiers, "standard/32", pool)
    assert rep.ok and fields(rep) == dict(count=16, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=1, first_bad_proof=NONE)
    exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
    r = subprocess.run([exe, "verify", "32"], cwd=ROOT, input="\n".join(proof_lines(32, pool[5])) + "\n", capture_output=True, text=True)
    assert "verified 1" in r.stdout, r.stdout + r.stderr


def positions(count):
    """first, last, and both sides of every wave (64) and fold-workgroup (256) edge inside the batch"""
    return sorted({p for p in (0, count - 1, 63, 64, 255, 256, count // 2) if 0 <= p < count})


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_counts_and_positions(lib, verifiers, pool, count):
    honest = pool[np.arange(count) % pool.shape[0]]
    assert both(lib, verifiers, "standard/32", honest).ok
    neg, off = row("standard/32", "neg_PI_Z")["proof"], row("standard/32", "off_curve_W_R")["proof"]
    h = verifiers["standard/32"]
    # the host twin bisects with host MSMs: it is asked for every position of the small batches, for the honest batch (above) of the large ones
    check = (lambda pr: both(lib, verifiers, "standard/32", pr)) if count <= 65 else (lambda pr: lib.plonk_verify_batch(h, pr, SEED, True))
    for p in positions(count):
        proofs = honest.copy()
        proofs[p] = neg
        rep = check(proofs)
        assert not rep.status.any()
        assert fields(rep) == dict(count=count, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=0, first_bad_proof=p), (p, fields(rep))
        q = count - 1 - p
        proofs = honest.copy()
        proofs[q] = off
        rep = check(proofs)
        assert [int(v) for v in np.nonzero(rep.status)[0]] == [q] and int(rep.status[q]) == BAD_POINT
        assert fields(rep) == dict(count=count, bad_status=1, first_bad_status=q, pairing_checked=1, pairing_ok=1, first_bad_proof=NONE), (q, fields(rep))
    assert lib.fault_stats()["slots_pending"] == 0


@pytest.mark.parametrize("circuit", ["standard/1024", "bool/14", "mimc/30", "extended/32", "zerowire/32"])
def test_every_widget_set_and_the_infinite_commitments(lib, verifiers, circuit):
    good = row(circuit, "none")["proof"]
    assert both(lib, verifiers, circuit, np.tile(good, (5, 1))).ok
    if circuit != "zerowire/32":
        proofs = np.tile(good, (5, 1))
        proofs[3] = row(circuit, "plus_one_linear_eval")["proof"]
        rep = both(lib, verifiers, circuit, proofs)
        assert not rep.ok and rep.first_bad_proof == 3


def test_sixteen_proofs_of_1024_gates_and_one_of_another_circuit(lib, verifiers):
    """the batch prover's 16 proofs of 2^10 gates are accepted; with one swapped for a valid proof of ANOTHER circuit of the same n the batch is
    rejected and the proof located"""
    from oracle.pyoracle import FR_MODULUS
    from barretenberg_amd.plonk import Prover, Verifier, bench_circuit, to_montgomery_limbs
    g2_x = fixture()[0]
    hs = lib.srs_generate(to_montgomery_limbs([SECRET % FR_MODULUS])[0], 2048)
    states = [bench_circuit(1024, 3 + 5 * k, 7 + 11 * k).preprocess() for k in range(16)]
    P = Prover(lib, states[0], hs)
    V = Verifier.from_prover(P, g2_x)
    try:
        proofs = P.construct_proofs([(s["w_l"], s["w_r"], s["w_o"]) for s in states])
        rep = V.verify(proofs, SEED, locate=True)
        assert rep.ok and whole(rep) == whole(V.verify(proofs, SEED, locate=True, host=True))
        # another circuit of the same n: the same chain, 24 gates shorter, padded to the same 1024 rows; its proof is valid THERE
        other = bench_circuit(1000, 3, 7).preprocess()
        assert other["n"] == states[0]["n"] == 1024
        Q = Prover(lib, other, hs)
        VQ = Verifier.from_prover(Q, g2_x)
        foreign = Q.construct_proof()
        Q.destroy()
        swapped = proofs.copy()
        swapped[9] = foreign
        rep = V.verify(swapped, SEED, locate=True)
        assert not rep.ok and fields(rep) == dict(count=16, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=0, first_bad_proof=9)
        assert whole(rep) == whole(V.verify(swapped, SEED, locate=True, host=True))
        VQ.destroy()
    finally:
        V.destroy()
        P.destroy()
        lib.srs_release(hs)


def test_one_seed_one_report(lib, verifiers, pool):
    proofs = pool.copy()
    proofs[7] = row("standard/32", "double_T_HI")["proof"]
    runs = [whole(lib.plonk_verify_batch(verifiers["standard/32"], proofs, SEED, True)) for _ in range(2)]
    assert runs[0] == runs[1] and runs[0]["first_bad_proof"] == 7
    other = lib.plonk_verify_batch(verifiers["standard/32"], proofs, SEED + np.uint64(1), True)
    assert fields(other) == {k: runs[0][k] for k in fields(other)} and whole(other)["a"] != runs[0]["a"] and whole(other)["b"] != runs[0]["b"]
    drawn = [lib.plonk_verify_batch(verifiers["standard/32"], pool) for _ in range(2)]
    assert all(r.ok for r in drawn) and list(drawn[0].seed) != list(drawn[1].seed)


def test_funnel_passes_of_a_warm_call(lib, verifiers, pool):
    seen = {}
    for count in (2, 257, 1000):
        proofs = pool[np.arange(count) % pool.shape[0]]
        assert lib.plonk_verify_batch(verifiers["standard/32"], proofs, SEED).ok  # warm
        lib.fault_inject("launch:%d" % FAR)
        assert lib.plonk_verify_batch(verifiers["standard/32"], proofs, SEED).ok
        seen[count] = lib.fault_stats()
        lib.fault_inject(None)
    print("funnel passes per warm call:", {c: {k: st[k] for k in WARM} for c, st in seen.items()})
    for count, st in seen.items():
        assert {k: st[k] for k in WARM} == WARM, (count, st)
    before = lib.memory_stats()["staging_bytes"]
    assert before >= 1000 * 2436  # the call's buffers are library staging


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, verifiers, pool, kind):
    """every site of the funnel `kind` that one warm call (LOCATE, one bad proof: fold and MSM rounds included) passes, failed once: an error return, no
    MSM slot pending, the live allocations of before, and the very next call correct"""
    from barretenberg_amd import BbGpuError
    proofs = pool.copy()
    proofs[11] = row("standard/32", "neg_W_O")["proof"]
    h = verifiers["standard/32"]
    want = whole(lib.plonk_verify_batch(h, proofs, SEED, True))  # warm
    assert want["first_bad_proof"] == 11
    lib.fault_inject("%s:%d" % (kind, FAR))
    assert whole(lib.plonk_verify_batch(h, proofs, SEED, True)) == want
    st = lib.fault_stats()
    sites = {"alloc": st["alloc_calls"], "h2d": st["h2d_calls"], "d2h": st["d2h_calls"], "launch": st["launch_checks"]}[kind]
    live = st["live_allocations"]
    assert sites >= {"alloc": 0, "h2d": 2, "d2h": 1, "launch": 4}[kind], st
    for k in range(sites):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError):
            lib.plonk_verify_batch(h, proofs, SEED, True)
        st = lib.fault_stats()
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["slots_pending"] == 0 and st["live_allocations"] == live, (kind, k, st)
        assert whole(lib.plonk_verify_batch(h, proofs, SEED, True)) == want, (kind, k)
    lib.fault_inject(None)


def test_the_stage_timing_of_the_last_call(lib, verifiers, pool):
    """bbgpu_plonk_verify_last_timing (diagnostic): the stages of the last call are non-negative wall times that add up to its total; with LOCATE
    the fold and MSM stages are sums over the rounds, so a located failure spends more there than the same batch without LOCATE"""
    proofs = pool.copy()
    proofs[3] = row("standard/32", "neg_Z_1")["proof"]
    h = verifiers["standard/32"]
    assert not lib.plonk_verify_batch(h, proofs, SEED).ok  # warm
    t0 = __import__("time").perf_counter()
    assert not lib.plonk_verify_batch(h, proofs, SEED).ok
    wall = (__import__("time").perf_counter() - t0) * 1e3
    plain = lib.plonk_verify_last_timing()
    assert all(v >= 0 for v in plain.values()) and 0 < plain["total_ms"] <= wall
    assert abs(plain["total_ms"] - sum(v for k, v in plain.items() if k != "total_ms")) < 1e-6
    assert plain["terms_ms"] > 0 and plain["msm_ms"] > 0 and plain["host_tail_ms"] > 0
    assert lib.plonk_verify_batch(h, proofs, SEED, True).first_bad_proof == 3
    located = lib.plonk_verify_last_timing()
    assert located["msm_ms"] > plain["msm_ms"] and located["host_tail_ms"] > plain["host_tail_ms"]  # five rounds against one
