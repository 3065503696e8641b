"""GPU tests (-m gpu) of the witness check of the resident prover: bbgpu_plonk_check_witness / _check_witness_batch (poly.hip k_check_gates_lanes / k_check_copies_lanes,
single and lane-batched), the opt-in gate bbgpu_plonk_set_witness_check in front of construct_proof / construct_proof_batch, and their funnel counts.
Three bars: (1) every GPU report equals the host entry's for the same witness, field by field (the host entry is held to the plain-Python model in
tests/test_plonk_check_host.py); (2) the REFERENCE'S VERIFIER judges the definition: a proof made with the check off verifies iff the report is all-clear;
(3) flag off is the old path, funnel for funnel."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FR_MODULUS, PolyOracle as P
from tests import plonk_check_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECRET_RAW = 0x0123456789ABCDEF_0F1E2D3C4B5A6978_FEDCBA9876543210_0123456789ABCDEF  # oracle/plonk_driver.cpp secret(), limbs 3..0
ERR_HIP, ERR_WITNESS = -1, -6
FUNNELS = ("alloc_calls", "h2d_calls", "d2h_calls", "launch_checks")


@pytest.fixture(scope="module")
def gpu():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


@pytest.fixture(scope="module")
def srs_for(gpu):
    made = {}

    def get(n):
        size = max(n, 65536)
        if size not in made:
            made[size] = gpu.srs_generate(P.mont([SECRET_RAW % FR_MODULUS])[0], size)
        return made[size]
    yield get
    for h in made.values():
        gpu.srs_release(h)


def host(gpu, state):
    from barretenberg_amd.plonk import host_check_witness
    return host_check_witness(state, gpu)


def same(got, want):
    return {k: got[k] for k in K.FIELDS} == {k: want[k] for k in K.FIELDS}


# 1. the GPU reports are the host entry's ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.ALL_CIRCUITS + ("mimc_64",))
def test_reports_equal_the_host_entry(gpu, srs_for, name):
    from barretenberg_amd.plonk import Prover
    state = K.circuit(name)
    cases = K.cases(name, state)
    own = [c for c in cases if not c.circuit_changed]  # same circuit, other wire values: one handle serves them all
    want = [host(gpu, c.state) for c in own]
    assert K.is_clear(want[0]) == (name != "mimc_64") and any(not K.is_clear(w) for w in want)
    A = Prover(gpu, state, srs_for(state["n"]))
    try:
        for c, w in zip(own, want):
            A.set_witness(*c.witness())
            got = A.check_witness()
            print(name, c.name, got)
            assert same(got, w), (name, c.name, got, w)
            assert A.check_witness() == got
        A.set_witness(*own[1].witness())
        for count, shift in ((1, 1), (3, 0), (8, 2), (16, 5), (3, 4)):
            lanes = [(shift + 3 * j) % len(own) for j in range(count)]  # honest and perturbed witnesses mixed in ONE call
            got, raw = A.check_witnesses([own[i].witness() for i in lanes], raw=True)
            for lane, i in enumerate(lanes):
                assert same(got[lane], want[i]), (name, count, lane, own[i].name, got[lane], want[i])
                assert same(A.last_witness_report(lane), want[i])
            again, raw2 = A.check_witnesses([own[i].witness() for i in lanes], raw=True)
            assert raw2 == raw and again == got
        assert same(A.check_witness(), want[1]), "the batch form left the handle's own witness alone"
    finally:
        A.destroy()
    for c in cases:
        if c.circuit_changed:  # a redirected mapping entry is another circuit: a handle of its own
            B = Prover(gpu, c.state, srs_for(state["n"]))
            try:
                w = host(gpu, c.state)
                got = B.check_witness()
                assert same(got, w), (name, c.name, got, w)
                assert same(B.check_witnesses([c.witness()] * 2)[1], w)
            finally:
                B.destroy()


def test_reports_at_2_20_gates(gpu, srs_for, golden):
    from barretenberg_amd.plonk import Prover, bench_circuit
    tr = golden("plonk_trace.json")
    state = bench_circuit(1 << 20, int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)).preprocess()
    n = state["n"]
    assert n == 1 << 20
    rinv = pow(1 << 256, -1, FR_MODULUS)
    rows = (12345, n // 2 + 7, n - 70000)
    bad = K.with_wires(state, [(2, r, K.raw_ints(state["w_o"][r:r + 1])[0] * rinv + 1) for r in rows])
    w_ok, w_bad = host(gpu, state), host(gpu, bad)
    assert K.is_clear(w_ok) and w_bad["gate_failures"] >= 3 and w_bad["first_gate"] <= rows[0]
    A = Prover(gpu, state, srs_for(n))
    try:
        assert same(A.check_witness(), w_ok)
        got = A.check_witnesses([K.Case("bad", bad).witness(), K.Case("ok", state).witness()])
        assert same(got[0], w_bad) and same(got[1], w_ok), got
        A.set_witness(*K.Case("bad", bad).witness())
        assert same(A.check_witness(), w_bad)
    finally:
        A.destroy()


# 2. the reference's Verifier is the judge of the definition ---------------------------------------------------------------------------------------------------
def _verified(lines, gates, **env):
    exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "transcript.dat")):
        pytest.fail("oracle/_ref/plonk_cpu (or its transcript) is missing: the reference's Verifier is the judge of this test")
    r = subprocess.run([exe, "verify", str(gates)], input="\n".join(lines) + "\n", cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="16", **env))
    out = r.stdout.strip()
    assert (r.returncode, out) in ((0, "verified 1"), (2, "verified 0")), (r.returncode, r.stdout, r.stderr[-500:])
    return out == "verified 1"


def _judged(golden, name):
    """-> (state, gates, verify environment, proof_lines keywords, golden proof lines or None)"""
    from barretenberg_amd.plonk import bench_circuit
    tr = golden("plonk_trace.json")
    kind, gates = name.split("_")
    if kind == "bench":
        state = bench_circuit(int(gates), int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)).preprocess()
        return state, int(gates), {}, {}, golden("plonk_proofs.json")["proofs"][gates][:26]
    state = K.circuit(name)
    if kind == "bool":
        return state, int(gates), {"BB_CIRCUIT": "bool"}, {}, tr["bool"]["proofs"][gates][:26]
    if kind == "mimc":
        gold = tr["mimc"]["proofs"].get(gates)
        return state, int(gates), {"BB_CIRCUIT": "mimc"}, {"mimc": True}, gold[:28] if gold else None
    assert kind == "ext"
    return state, int(gates), {"BB_CIRCUIT": "extended"}, {"sequential": True}, tr["extended"]["proofs"][gates][:27]


@pytest.mark.parametrize("name", ["bench_1024", "bench_65536", "bool_4096", "mimc_4094", "ext_160", "mimc_63", "mimc_64"])
def test_reference_verifier_agrees_with_the_report(gpu, srs_for, golden, name):
    from barretenberg_amd.plonk import Prover, proof_lines
    state, gates, env, kw, gold = _judged(golden, name)
    tried = {c.name: c for c in K.cases(name, state) if not c.circuit_changed} if name != "mimc_64" else {"honest": K.Case("honest", state)}
    pick = ("honest", "row_n-2") if name == "mimc_63" else ("honest",) if name == "mimc_64" else ("honest", "middle_row", "row_n-1_only", "representatives")
    A = Prover(gpu, state, srs_for(state["n"]))
    verdicts = {}
    try:
        for cname in pick:
            c = tried[cname]
            A.set_witness(*c.witness())
            rep = A.check_witness()
            lines = proof_lines(state["n"], A.construct_proof(), **kw)  # the check is OFF: the prover takes what it is given
            ok = _verified(lines, gates, **env)
            verdicts[cname] = (ok, rep["gate_failures"], rep["copy_failures"])
            print(name, cname, "verified", ok, rep)
            assert ok == K.is_clear(rep), (name, cname, ok, rep)
            if gold is not None and cname in ("honest", "representatives"):  # any representative below 2^256 is the prover's input convention
                assert lines == gold, (name, cname)
    finally:
        A.destroy()
    if name == "mimc_64":  # the reference's own quirk: its Verifier rejects the honest proof of a MiMC circuit of exactly 2^k gates
        assert verdicts["honest"] == (False, 0, 2)
    elif name == "mimc_63":
        assert verdicts["honest"][0] and not verdicts["row_n-2"][0]
    else:
        assert verdicts["honest"][0] and verdicts["row_n-1_only"][0] and verdicts["representatives"][0] and not verdicts["middle_row"][0]


# 3. the opt-in gate -------------------------------------------------------------------------------------------------------------------------------------------
class Bench1024:
    def __init__(self, gpu, srs, gates=1024):
        from barretenberg_amd.plonk import Prover, bench_circuit
        self.states = [bench_circuit(gates, K.A0 + j, K.B0 + 3 * j).preprocess() for j in range(8)]
        self.n = self.states[0]["n"]
        self.ws = [tuple(s[k] for k in K.WIRES) for s in self.states]
        self.A = Prover(gpu, self.states[0], srs)
        self.S = Prover(gpu, self.states[0], srs)
        self.one = []
        for w in self.ws:
            self.S.set_witness(*w)
            self.one.append(self.S.construct_proof())

    def perturbed(self, j):
        M = K.Model(self.states[j])
        row = self.n // 3
        assert M.q["q_o"][row]
        st = K.with_wires(self.states[j], [(2, row, M.w[2][row] + 1)])
        return st, tuple(st[k] for k in K.WIRES)

    def destroy(self):
        self.A.destroy()
        self.S.destroy()


def _raw_batch(gpu, prover, ws, fill=0xA5):
    """the batch entry with a pre-filled output buffer -> (return code, the buffer)"""
    L = gpu.lib
    keep = [[np.ascontiguousarray(a, dtype=np.uint64) for a in w] for w in ws]
    cols = [(C.c_void_p * len(ws))(*[w[k].ctypes.data for w in keep]) for k in range(3)]
    out = np.full((len(ws), 120), fill * 0x0101010101010101, dtype=np.uint64)
    L.bbgpu_plonk_construct_proof_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L.bbgpu_plonk_construct_proof_batch(prover.handle, len(ws), cols[0], cols[1], cols[2], out.ctypes.data), out


def _raw_single(gpu, prover, fill=0xA5):
    out = np.full(120, fill * 0x0101010101010101, dtype=np.uint64)
    return gpu.lib.bbgpu_plonk_construct_proof(prover.handle, out.ctypes.data_as(C.POINTER(C.c_uint64))), out


def test_opt_in_gate(gpu, srs_for):
    from barretenberg_amd.plonk import WitnessError
    B = Bench1024(gpu, srs_for(1024))
    try:
        A = B.A
        off = A.construct_proofs(B.ws)
        A.set_witness(*B.ws[3])
        off1 = A.construct_proof()
        assert all(np.array_equal(off[j], B.one[j]) for j in range(8)) and np.array_equal(off1, B.one[3])
        A.set_witness_check(True)
        assert np.array_equal(A.construct_proofs(B.ws), off), "an all-honest batch with the check on"
        assert all(K.is_clear(A.last_witness_report(j)) for j in range(8))
        assert np.array_equal(A.construct_proof(), off1), "an honest witness with the check on"
        assert K.is_clear(A.last_witness_report(0))
        # lanes 2 and 5 perturbed
        bad = {j: B.perturbed(j) for j in (2, 5)}
        ws = [bad[j][1] if j in bad else B.ws[j] for j in range(8)]
        rc, out = _raw_batch(gpu, A, ws)
        assert rc == ERR_WITNESS, (rc, gpu.lib.bbgpu_last_error())
        msg = gpu.lib.bbgpu_last_error().decode()
        assert "lane 2" in msg and "row %d" % (B.n // 3) in msg, msg
        assert np.all(out == np.uint64(0xA5A5A5A5A5A5A5A5)), "no proof bytes for any lane"
        assert gpu.fault_stats()["slots_pending"] == 0
        for j in range(8):
            rep = A.last_witness_report(j)
            if j in bad:
                assert same(rep, host(gpu, bad[j][0])) and not K.is_clear(rep), (j, rep)
            else:
                assert K.is_clear(rep), (j, rep)
        with pytest.raises(WitnessError) as e:
            A.construct_proofs(ws)
        assert e.value.bad_lanes() == [2, 5] and len(e.value.reports) == 8
        good = [j for j in range(8) if j not in bad]
        six = A.construct_proofs([B.ws[j] for j in good])  # the same handle proves the six good lanes
        for lane, j in enumerate(good):
            assert np.array_equal(six[lane], B.one[j]), (lane, j)
        # the single entry
        A.set_witness(*bad[5][1])
        rc, out = _raw_single(gpu, A)
        assert rc == ERR_WITNESS and np.all(out == np.uint64(0xA5A5A5A5A5A5A5A5)) and gpu.fault_stats()["slots_pending"] == 0
        assert "lane 0" in gpu.lib.bbgpu_last_error().decode()
        assert same(A.last_witness_report(0), host(gpu, bad[5][0]))
        with pytest.raises(WitnessError):
            A.construct_proof()
        A.set_witness(*B.ws[5])
        assert np.array_equal(A.construct_proof(), B.one[5])
        A.set_witness_check(False)  # off again: the prover takes what it is given
        A.set_witness(*bad[5][1])
        rc, out = _raw_single(gpu, A)
        assert rc == 0 and not np.array_equal(out, B.one[5])
    finally:
        B.destroy()


# 4. funnel counts -----------------------------------------------------------------------------------------------------------------------------------------------
def _funnels(gpu, run):
    s0 = gpu.fault_stats()
    run()
    s1 = gpu.fault_stats()
    return {k: s1[k] - s0[k] for k in FUNNELS}


def test_funnel_counts_flag_off_is_the_old_path_and_the_check_is_lane_batched(gpu, srs_for):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.plonk import Prover, WitnessError
    B = Bench1024(gpu, srs_for(1 << 14), gates=1 << 14)
    T = Prover(gpu, B.states[0], srs_for(1 << 14))  # its flag is set and cleared again; B.A's is never touched
    try:
        T.set_witness_check(True)
        T.set_witness_check(False)
        count = {}
        for label, X in (("untouched", B.A), ("toggled", T)):
            X.construct_proofs(B.ws)  # warm: lanes, tables, workspaces
            X.construct_proof()
            count[label] = (_funnels(gpu, X.construct_proof), _funnels(gpu, lambda: X.construct_proofs(B.ws)))
        print("funnels, flag off: single %s, batch of 8 %s" % count["untouched"])
        assert count["untouched"] == count["toggled"]
        T.set_witness_check(True)
        T.construct_proof()  # the first checked calls allocate the 640 bytes of result records
        T.construct_proofs(B.ws)
        on = (_funnels(gpu, T.construct_proof), _funnels(gpu, lambda: T.construct_proofs(B.ws)))
        print("funnels, flag on:  single %s, batch of 8 %s" % on)
        extra = [on[i]["launch_checks"] - count["toggled"][i]["launch_checks"] for i in (0, 1)]
        assert extra[0] == extra[1] and 0 < extra[0] <= 4, extra  # two launches, not two per lane
        assert on[0]["alloc_calls"] == count["toggled"][0]["alloc_calls"] and on[1]["alloc_calls"] == count["toggled"][1]["alloc_calls"]
        # an injected failure of the check's own launch / copy-back is a HIP error, not a verdict
        want1 = T.construct_proof()
        want8 = T.construct_proofs(B.ws)
        for spec in ("launch:0", "launch:1", "d2h:0"):
            for single in (True, False):
                gpu.fault_inject(spec)
                rc, out = _raw_single(gpu, T) if single else _raw_batch(gpu, T, B.ws)
                st = gpu.fault_stats()
                gpu.fault_inject(None)
                assert rc == ERR_HIP, (spec, single, rc, gpu.lib.bbgpu_last_error())
                assert st["fired"] == 1 and st["slots_pending"] == 0, (spec, st)
                assert np.all(out == np.uint64(0xA5A5A5A5A5A5A5A5)), (spec, single)
                assert np.array_equal(T.construct_proof(), want1) if single else np.array_equal(T.construct_proofs(B.ws), want8)
        assert BbGpuError is not WitnessError
    finally:
        T.destroy()
        B.destroy()


def test_check_entries_refuse_bad_arguments_before_a_device_is_needed(gpu, srs_for):
    from barretenberg_amd.bbgpu import WitnessReport
    from barretenberg_amd.plonk import Prover
    state = K.circuit("bench_64")
    A = Prover(gpu, state, srs_for(64))
    try:
        L = gpu.lib
        L.bbgpu_plonk_check_witness_batch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.bbgpu_plonk_check_witness.argtypes = [C.c_int, C.c_void_p]
        reps = (WitnessReport * 17)()
        w = [np.ascontiguousarray(state[k]) for k in K.WIRES]
        cols = [(C.c_void_p * 17)(*[a.ctypes.data] * 17) for a in w]
        assert L.bbgpu_plonk_check_witness_batch(A.handle, 0, cols[0], cols[1], cols[2], reps) == -3
        assert L.bbgpu_plonk_check_witness_batch(A.handle, 17, cols[0], cols[1], cols[2], reps) == -3
        assert L.bbgpu_plonk_check_witness_batch(A.handle, 2, cols[0], None, cols[2], reps) == -3
        assert L.bbgpu_plonk_check_witness_batch(A.handle, 2, cols[0], cols[1], cols[2], None) == -3
        assert L.bbgpu_plonk_check_witness_batch(12345, 2, cols[0], cols[1], cols[2], reps) == -3
        assert L.bbgpu_plonk_check_witness(A.handle, None) == -3
        assert L.bbgpu_plonk_check_witness_batch(A.handle, 16, cols[0], cols[1], cols[2], reps) == 0
        assert all(K.is_clear(reps[j].as_dict()) for j in range(16))
    finally:
        A.destroy()
