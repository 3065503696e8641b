"""bbgpu_plonk_verify_multi on the GPU (-m gpu): proofs of several circuits in one batch -- k_verify_terms<true> reads each thread's circuit from a
record, k_verify_fold<true> sums a circuit's shared terms in workgroup (slot, circuit), A and B are two device MSMs, one pairing tail for all.  Every
report is compared, field for field and with status, a and b, with bbgpu_host_plonk_verify_multi on the same batch; expected verdicts come from the
reference's verdicts on the rows (tests/golden/plonk_verify.json) or from what a tamper changes (tests/plonk_verify_multi_cases.tampered), never from
this code's own answer.  Shapes are small on purpose: less than a wave, three waves with the last partial, and the fold's strided loop past 2 x 256."""
import numpy as np
import pytest

from tests.plonk_verify_cases import BAD_POINT, NONE, SEED, fields, fixture, row, whole
from tests.plonk_verify_multi_cases import (CIRCUITS, honest, honest_batch, index, keys, other_g2, others_plus, place, round_robin,
                                            sorted_then_round_robin, tampered)

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
FAR = 1 << 62
ERR_ARG, ERR_SIZE = -3, -2


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def handles(lib):
    """one handle per circuit of the fixture, in CIRCUITS' order, made once"""
    g2_x, circuits, _ = fixture()
    hs = [lib.plonk_verifier_create(circuits[c]["n"], circuits[c]["widgets"], circuits[c]["vk"], g2_x) for c in CIRCUITS]
    yield hs
    for h in hs:
        lib.plonk_verifier_destroy(h)


def both(lib, handles, labels, proofs, names=CIRCUITS, seed=SEED, locate=True):
    """the GPU report and the host twin's of one batch; they must agree in every field, status, a and b included"""
    gpu = lib.plonk_verify_multi([handles[index(c)] for c in names], labels, proofs, seed, locate)
    host = lib.host_plonk_verify_multi(keys(names), fixture()[0], labels, proofs, seed, locate)
    assert whole(gpu) == whole(host), (fields(gpu), fields(host), list(gpu.status), list(host.status))
    assert lib.fault_stats()["slots_pending"] == 0
    return gpu


def good(count):
    return dict(count=count, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=1, first_bad_proof=NONE)


def expect(count, position, bad):
    """the fields of a batch of honest proofs with `bad` at `position`: an off-curve point is flagged by its status and leaves the sums; the other
    tampers keep status 0 and fail the pairing, where LOCATE finds them"""
    if "off_curve" in bad:
        return dict(good(count), bad_status=1, first_bad_status=position)
    return dict(good(count), pairing_ok=0, first_bad_proof=position)


TAMPERS = ("neg_T_LO of standard/32", "plus_one_w_o_shifted_eval of extended/32", "off_curve_W_R of bool/14", "plus_one_q_mimc_coefficient_eval of mimc/30")


def test_seven_proofs_less_than_a_wave_every_record_used(lib, handles):
    labels = np.array([0, 1, 2, 3, 4, 5, 3], dtype=np.uint32)
    rep = both(lib, handles, labels, honest_batch(labels))
    assert rep.ok and fields(rep) == good(7)


@pytest.fixture(scope="module")
def batch130():
    labels = round_robin(130)
    proofs = honest_batch(labels)
    proofs.setflags(write=False)
    return labels, proofs


def test_130_proofs_round_robin(lib, handles, batch130):
    """every wave holds all four values of log2 n and all four widget sets; the last wave is partial"""
    rep = both(lib, handles, *batch130)
    assert rep.ok and fields(rep) == good(130)


@pytest.mark.parametrize("position", [0, 63, 64, 129])
@pytest.mark.parametrize("which", range(4), ids=[t.split()[0] for t in TAMPERS])
def test_130_proofs_one_tampered_and_located(lib, handles, batch130, which, position):
    labels, proofs = place(*batch130, position, tampered()[which])
    rep = both(lib, handles, labels, proofs)
    assert fields(rep) == expect(130, position, TAMPERS[which]), (TAMPERS[which], position)
    assert [int(v) for v in np.nonzero(rep.status)[0]] == ([position] if "off_curve" in TAMPERS[which] else [])
    if "off_curve" in TAMPERS[which]:
        assert int(rep.status[position]) == BAD_POINT


def test_600_proofs_sorted_then_round_robin(lib, handles):
    """the first 300 sorted by circuit, the rest round-robin: the fold's strided loop runs past 2 x 256 over runs and gaps of every circuit's mask;
    then one tampered proof at 511"""
    labels = sorted_then_round_robin(600, 300)
    proofs = honest_batch(labels)
    rep = both(lib, handles, labels, proofs)
    assert rep.ok and fields(rep) == good(600)
    labels, proofs = place(labels, proofs, 511, tampered()[1])
    assert fields(both(lib, handles, labels, proofs)) == expect(600, 511, TAMPERS[1])


def test_a_wrong_label_is_a_bad_proof(lib, handles):
    r = row("standard/32", "proof_of_extended_32")
    labels, proofs, p = others_plus(dict(r, circuit="extended/32"), "middle")
    assert both(lib, handles, labels, proofs).ok
    labels = labels.copy()
    labels[p] = index("standard/32")
    assert fields(both(lib, handles, labels, proofs)) == expect(6, p, "wrong label")


def test_exchanged_labels_of_two_circuits_of_the_same_n(lib, handles):
    proofs = np.stack([honest("standard/32"), honest("mimc/30")])
    right = np.array([index("standard/32"), index("mimc/30")], dtype=np.uint32)
    assert both(lib, handles, right, proofs).ok
    assert fields(both(lib, handles, right[::-1].copy(), proofs)) == expect(2, 0, "exchanged")


@pytest.mark.parametrize("circuit", ["standard/32", "extended/32"])
def test_one_circuit_and_duplicate_handles_equal_the_single_circuit_entry(lib, handles, circuit):
    """G = 1 is bbgpu_plonk_verify_batch's definition; [h, h] with the labels alternating gives its a, b and verdict too: the segmented sums against
    the plain one, on the GPU"""
    h = handles[index(circuit)]
    proofs = honest_batch(np.full(70, index(circuit)))
    for bad in (None, "neg_Z_1"):
        if bad:
            proofs[66] = row(circuit, bad)["proof"]
        one = lib.plonk_verify_batch(h, proofs, SEED, True)
        assert one.ok == (bad is None) and int(one.first_bad_proof) == (NONE if bad is None else 66)
        assert whole(lib.plonk_verify_multi([h], np.zeros(70, dtype=np.uint32), proofs, SEED, True)) == whole(one)
        assert whole(lib.plonk_verify_multi([h, h], (np.arange(70) % 2).astype(np.uint32), proofs, SEED, True)) == whole(one)
        assert whole(lib.plonk_verify_multi([h, h, h], (np.arange(70) % 3).astype(np.uint32), proofs, SEED, False)) == \
            whole(lib.plonk_verify_batch(h, proofs, SEED, False))
    assert lib.fault_stats()["slots_pending"] == 0


def test_a_second_verifier_without_proofs_changes_nothing(lib, handles):
    """seven proofs of standard/32, all labelled 0, beside a verifier of more shared rows that gets none: the mixed fold over an empty circuit writes
    zeros on that circuit's rows, so the report is the one-verifier call's bit for bit, and the host twin's"""
    labels = np.zeros(7, dtype=np.uint32)
    proofs = honest_batch(np.full(7, index("standard/32")))
    proofs[5] = row("standard/32", "neg_Z_1")["proof"]
    one = lib.plonk_verify_multi([handles[index("standard/32")]], labels, proofs, SEED, True)
    assert not one.ok and int(one.first_bad_proof) == 5
    assert whole(both(lib, handles, labels, proofs, names=["standard/32", "extended/32"])) == whole(one)


def test_one_seed_one_report(lib, handles, batch130):
    labels, proofs = place(*batch130, 77, tampered()[3])
    hs = handles
    runs = [whole(lib.plonk_verify_multi(hs, labels, proofs, SEED, True)) for _ in range(2)]
    assert runs[0] == runs[1] and runs[0]["first_bad_proof"] == 77
    other = lib.plonk_verify_multi(hs, labels, proofs, SEED + np.uint64(1), True)
    assert fields(other) == {k: runs[0][k] for k in fields(other)} and whole(other)["a"] != runs[0]["a"] and whole(other)["b"] != runs[0]["b"]
    drawn = [lib.plonk_verify_multi(hs, *batch130) for _ in range(2)]
    assert all(r.ok for r in drawn) and list(drawn[0].seed) != list(drawn[1].seed)


def test_funnel_passes_of_a_warm_call_equal_the_single_circuit_entrys(lib, handles, batch130):
    """130 proofs of six circuits pass as many allocation / upload / read-back / launch checks as 130 proofs of one through bbgpu_plonk_verify_batch"""
    labels, proofs = batch130
    single = honest_batch(np.zeros(130, dtype=np.uint32))
    calls = {"multi": lambda: lib.plonk_verify_multi(handles, labels, proofs, SEED), "batch": lambda: lib.plonk_verify_batch(handles[0], single, SEED)}
    seen = {}
    for name, call in calls.items():
        assert call().ok  # warm
        lib.fault_inject("launch:%d" % FAR)
        assert call().ok
        st = lib.fault_stats()
        lib.fault_inject(None)
        assert st["slots_pending"] == 0
        seen[name] = {k: st[k] for k in ("alloc_calls", "h2d_calls", "d2h_calls", "launch_checks")}
    print("funnel passes per warm call:", seen)
    assert seen["multi"] == seen["batch"] == dict(alloc_calls=0, h2d_calls=2, d2h_calls=1, launch_checks=4)
    t = lib.plonk_verify_last_timing()  # the last call of either entry
    assert t["total_ms"] > 0 and abs(t["total_ms"] - sum(v for k, v in t.items() if k != "total_ms")) < 1e-6


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind(lib, handles, kind):
    """every site of the funnel `kind` that one warm mixed call (LOCATE, one bad proof: fold and MSM rounds included) passes, failed once by the
    library's simulated error return: an error code, no MSM slot pending, the live allocations of before, and the very next call correct"""
    from barretenberg_amd import BbGpuError
    labels = round_robin(20)
    labels, proofs = place(labels, honest_batch(labels), 11, tampered()[0])
    want = whole(lib.plonk_verify_multi(handles, labels, proofs, SEED, True))  # warm
    assert want["first_bad_proof"] == 11
    lib.fault_inject("%s:%d" % (kind, FAR))
    assert whole(lib.plonk_verify_multi(handles, labels, proofs, SEED, True)) == want
    st = lib.fault_stats()
    sites = {"alloc": st["alloc_calls"], "h2d": st["h2d_calls"], "d2h": st["d2h_calls"], "launch": st["launch_checks"]}[kind]
    live = st["live_allocations"]
    assert sites >= {"alloc": 0, "h2d": 2, "d2h": 1, "launch": 4}[kind], st
    for k in range(sites):
        lib.fault_inject("%s:%d" % (kind, k))
        with pytest.raises(BbGpuError):
            lib.plonk_verify_multi(handles, labels, proofs, SEED, True)
        st = lib.fault_stats()
        assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
        assert st["slots_pending"] == 0 and st["live_allocations"] == live, (kind, k, st)
        assert whole(lib.plonk_verify_multi(handles, labels, proofs, SEED, True)) == want, (kind, k)
    lib.fault_inject(None)


def test_argument_errors_pass_no_funnel(lib, handles, batch130):
    """refused before any device work: the code, a text, and not one allocation, copy or launch check"""
    from barretenberg_amd import BbGpuError
    labels, proofs = batch130
    g2_x, circuits, _ = fixture()
    c = circuits["standard/32"]
    foreign = lib.plonk_verifier_create(c["n"], c["widgets"], c["vk"], other_g2())
    bad_labels = labels.copy()
    bad_labels[129] = 6
    big = (1 << 14) + 1
    cases = [(ERR_ARG, [], labels, proofs), (ERR_SIZE, handles * 11, labels, proofs), (ERR_ARG, handles[:5] + [1 << 20], labels, proofs),
             (ERR_ARG, handles, bad_labels, proofs), (ERR_ARG, handles[:5] + [foreign], labels, proofs), (ERR_ARG, handles, labels[:0], proofs[:0]),
             (ERR_SIZE, handles, np.zeros(big, dtype=np.uint32), np.zeros((big, 120), dtype=np.uint64))]
    lib.fault_inject("launch:%d" % FAR)
    try:
        for want, hs, lb, pr in cases:
            with pytest.raises(BbGpuError) as e:
                lib.plonk_verify_multi(hs, lb, pr, SEED)
            words = str(e.value).split()
            assert int(words[2].rstrip(":")) == want and len(words) > 3, str(e.value)
        with pytest.raises(BbGpuError, match=r"circuit\[129\]"):
            lib.plonk_verify_multi(handles, bad_labels, proofs, SEED)
        st = lib.fault_stats()
        assert (st["alloc_calls"], st["h2d_calls"], st["d2h_calls"], st["launch_checks"]) == (0, 0, 0, 0), st
    finally:
        lib.fault_inject(None)
        lib.plonk_verifier_destroy(foreign)
    assert lib.plonk_verify_multi(handles, labels, proofs, SEED).ok
