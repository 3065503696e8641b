"""GPU tests (-m gpu) of bbgpu_plonk_construct_proof_batch: `count` proofs of one circuit in one resident call, the rounds in lockstep over the lanes
(plonk.hip, the lane-batched kernels of poly.hip).  The bar is the single-proof path's: every lane's proof is byte for byte what set_witness +
construct_proof return for that witness on a SECOND handle, lane 0 (the golden witness) equals the reference's golden proof, and the reference's own
Verifier accepts lanes of a batch.  Witness j of a batch is bench_circuit(gates, a0 + j, b0 + 3j): the same circuit with other wire values
(tests/test_plonk_batch_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pyoracle import FR_MODULUS, PolyOracle as P, to_int

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECRET_RAW = 0x0123456789ABCDEF_0F1E2D3C4B5A6978_FEDCBA9876543210_0123456789ABCDEF  # oracle/plonk_driver.cpp secret(), limbs 3..0
CH = ("gamma", "beta", "alpha", "z", "nu")


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


def hx(a):
    return ["%064x" % to_int(r) for r in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


class Bench:
    """the bench circuit at one size: a handle for batches, a second one for single proofs, witnesses and single proofs made on demand"""

    def __init__(self, gpu, srs, golden, gates):
        from barretenberg_amd.plonk import Prover, bench_circuit
        self.gates = gates
        tr = golden("plonk_trace.json")
        self.a0, self.b0 = int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)
        self.state = bench_circuit(gates, self.a0, self.b0).preprocess()
        self.n = self.state["n"]
        self.batch = Prover(gpu, self.state, srs)
        self.single = Prover(gpu, self.state, srs)
        self._w, self._one = {0: tuple(self.state[k] for k in ("w_l", "w_r", "w_o"))}, {}

    def witness(self, j):
        from barretenberg_amd.plonk import bench_circuit
        if j not in self._w:
            st = bench_circuit(self.gates, self.a0 + j, self.b0 + 3 * j).preprocess()
            self._w[j] = tuple(st[k] for k in ("w_l", "w_r", "w_o"))
        return self._w[j]

    def one(self, j):
        """(proof, challenges) of witness j from the single-proof path of the second handle"""
        if j not in self._one:
            self.single.set_witness(*self.witness(j))
            proof = self.single.construct_proof()
            self._one[j] = (proof, {k: v.copy() for k, v in self.single.challenges().items()})
        return self._one[j]

    def check(self, proofs, js):
        assert proofs.shape == (len(js), 120)
        for lane, j in enumerate(js):
            want, ch = self.one(j)
            assert np.array_equal(proofs[lane], want), ("lane", lane, "witness", j)
            got = self.batch.batch_challenges(lane)
            for name in CH:
                assert np.array_equal(got[name], ch[name]), (lane, name)

    def destroy(self):
        self.batch.destroy()
        self.single.destroy()


@pytest.fixture(scope="module")
def bench(gpu, srs_for, golden):
    made = {}

    def get(gates):
        if gates not in made:
            made[gates] = Bench(gpu, srs_for(gates), golden, gates)
        return made[gates]
    yield get
    for b in made.values():
        b.destroy()


def _verify(lines, gates, **env):
    exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
    if not os.path.exists(exe) or not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "transcript.dat")):
        pytest.fail("oracle/_ref/plonk_cpu (or its transcript) is missing: the reference's Verifier is the judge of this test")
    r = subprocess.run([exe, "verify", str(gates)], input="\n".join(lines) + "\n", cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OMP_NUM_THREADS="16", **env))
    assert r.returncode == 0 and r.stdout.strip() == "verified 1", (r.stdout, r.stderr[-500:])


# 3. bytes ---------------------------------------------------------------------------------------------------------------------------------------------
CASES = [(g, c) for g in (32, 1024, 16384, 65536) for c in (1, 2, 3, 5, 8, 16)] + [(1 << 18, 4), (1 << 20, 2), (1 << 21, 2)]


@pytest.mark.parametrize("gates,count", CASES)
def test_batch_proofs_are_byte_identical(bench, golden, gates, count):
    from barretenberg_amd.plonk import proof_lines
    B = bench(gates)
    js = list(range(count))
    proofs = B.batch.construct_proofs([B.witness(j) for j in js])
    assert proof_lines(B.n, proofs[0]) == golden("plonk_proofs.json")["proofs"][str(gates)][:26]
    tr = golden("plonk_trace.json")
    ch0 = B.batch.batch_challenges(0)
    for name in CH:
        assert hx(ch0[name])[0] == tr["challenges"][str(gates)][name], name
    B.check(proofs, js)
    if gates > 65536:  # 96 MiB x 4 per lane and handle at 2^18 gates and up: give it back before the next size
        B.destroy()


# 4. the reference judges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gates", [32, 1024, 16384, 65536])
def test_reference_verifier_accepts_lanes_of_a_batch(bench, gates):
    from barretenberg_amd.plonk import proof_lines
    B = bench(gates)
    proofs = B.batch.construct_proofs([B.witness(j) for j in range(8)])
    for lane in (0, 1, 7):
        _verify(proof_lines(B.n, proofs[lane]), gates)


# 5. lanes are independent -----------------------------------------------------------------------------------------------------------------------------
def test_lanes_are_independent(bench):
    B = bench(1024)
    js = [3, 0, 2, 1]
    a = B.batch.construct_proofs([B.witness(j) for j in range(4)])
    b = B.batch.construct_proofs([B.witness(j) for j in js])
    for lane, j in enumerate(js):
        assert np.array_equal(b[lane], a[j]), (lane, j)
    B.check(b, js)
    c = B.batch.construct_proofs([B.witness(1), B.witness(2), B.witness(1)])
    assert np.array_equal(c[0], c[2]) and not np.array_equal(c[0], c[1])
    B.check(c, [1, 2, 1])


def test_smaller_then_larger_count_on_one_handle(gpu, srs_for, golden):
    B = Bench(gpu, srs_for(1024), golden, 1024)
    try:
        for count in (4, 2, 7, 1):
            js = list(range(count))
            B.check(B.batch.construct_proofs([B.witness(j) for j in js]), js)
            assert B.batch.batch_timing()["total_ms"] > 0
    finally:
        B.destroy()


# 6. the single path is untouched ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gates", [32, 16384])
def test_single_proof_after_a_batch_is_unchanged(gpu, srs_for, golden, gates):
    from barretenberg_amd.plonk import proof_lines
    B = Bench(gpu, srs_for(gates), golden, gates)
    try:
        tr = golden("plonk_trace.json")
        gold = golden("plonk_proofs.json")["proofs"][str(gates)][:26]
        before = B.batch.construct_proof()
        ch_before = {k: v.copy() for k, v in B.batch.challenges().items()}
        t_before = B.batch.timing()
        B.batch.construct_proofs([B.witness(j) for j in (2, 1, 3)])  # lane 0 is NOT the handle's own witness
        after_ch = B.batch.challenges()
        for name in CH:
            assert np.array_equal(after_ch[name], ch_before[name]), name
        assert B.batch.timing() == t_before
        batch_ch = [{k: v.copy() for k, v in B.batch.batch_challenges(lane).items()} for lane in range(3)]
        batch_t = B.batch.batch_timing()
        after = B.batch.construct_proof()
        assert np.array_equal(after, before) and proof_lines(B.n, after) == gold
        for name in CH:
            assert hx(B.batch.challenges()[name])[0] == tr["challenges"][str(gates)][name], name
        # and the other way round: the single proof runs through the same rounds, and leaves what the batch reported alone
        for lane in range(3):
            got = B.batch.batch_challenges(lane)
            for name in CH:
                assert np.array_equal(got[name], batch_ch[lane][name]), (lane, name)
        assert B.batch.batch_timing() == batch_t
    finally:
        B.destroy()


# 7. widgets -------------------------------------------------------------------------------------------------------------------------------------------
def _widget_case(gpu, srs, states, gold, **lines_kw):
    """states: one circuit state per lane (the same circuit, possibly other wires); gold: {lane: golden proof lines}"""
    from barretenberg_amd.plonk import Prover, proof_lines
    A, S = Prover(gpu, states[0], srs), Prover(gpu, states[0], srs)
    try:
        proofs = A.construct_proofs([(s["w_l"], s["w_r"], s["w_o"]) for s in states])
        for lane, s in enumerate(states):
            S.set_witness(s["w_l"], s["w_r"], s["w_o"])
            assert np.array_equal(proofs[lane], S.construct_proof()), lane
            ch, want = A.batch_challenges(lane), S.challenges()
            for name in CH:
                assert np.array_equal(ch[name], want[name]), (lane, name)
        for lane, lines in gold.items():
            assert proof_lines(states[0]["n"], proofs[lane], **lines_kw) == lines, lane
    finally:
        A.destroy()
        S.destroy()


@pytest.mark.parametrize("gates", [6, 64, 4096])
def test_batch_with_bool_widget(gpu, srs_for, golden, gates):
    from barretenberg_amd.plonk import bool_circuit
    st = bool_circuit(gates).preprocess()
    gold = golden("plonk_trace.json")["bool"]["proofs"][str(gates)][:26]
    _widget_case(gpu, srs_for(65536), [st, st, st], {0: gold, 1: gold, 2: gold})


MIMC_X0 = 0x0777777788888888555555556666666633333333444444441111111122222222
MIMC_K = 0x0ABCDEFABCDEFABC1234123412341234DDDDEEEEFFFF00009999AAAABBBBCCCC


@pytest.mark.parametrize("gates", [6, 93, 4094])
def test_batch_with_mimc_widget(gpu, srs_for, golden, gates):
    from barretenberg_amd.plonk import mimc_circuit
    states = [mimc_circuit(gates, MIMC_X0 + j, MIMC_K).preprocess() for j in range(3)]
    for s in states[1:]:
        assert np.array_equal(s["q_mimc_coefficient"], states[0]["q_mimc_coefficient"]) and not np.array_equal(s["w_l"], states[0]["w_l"])
    gold = golden("plonk_trace.json")["mimc"]["proofs"][str(gates)][:28]
    _widget_case(gpu, srs_for(65536), states, {0: gold}, mimc=True)


@pytest.mark.parametrize("gates", [32, 160])
def test_batch_with_sequential_and_bool_widgets(gpu, srs_for, golden, gates):
    z = np.load(os.path.join(ROOT, "tests", "golden", "plonk_extended_state.npz"))
    st = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("%d/" % gates)}
    st["n"] = int(st["n"][0])
    gold = golden("plonk_trace.json")["extended"]["proofs"][str(gates)][:27]
    _widget_case(gpu, srs_for(65536), [st, st, st], {0: gold, 1: gold, 2: gold}, sequential=True)


# 8. commitments at infinity ---------------------------------------------------------------------------------------------------------------------------
def test_batch_commitments_at_infinity(gpu, srs_for):
    from barretenberg_amd.plonk import Prover, proof_lines, zero_wire_circuit
    a0 = 0x0777777788888888555555556666666633333333444444441111111122222222
    states = [zero_wire_circuit(32, a0 + j).preprocess() for j in range(3)]
    A = Prover(gpu, states[0], srs_for(65536))
    try:
        proofs = A.construct_proofs([(s["w_l"], s["w_r"], s["w_o"]) for s in states])
        for lane in range(3):
            lines = proof_lines(states[0]["n"], proofs[lane])
            got = dict(ln.split() for ln in lines[1:])
            for k in ("W_R", "W_O"):
                assert got[k + ".x"] == "0" * 64 and got[k + ".y"] == "8" + "0" * 63, (lane, k)
        assert not np.array_equal(proofs[0], proofs[1])
        _verify(proof_lines(states[0]["n"], proofs[1]), 32, BB_CIRCUIT="zerowire", BBGPU_SHIM_STRICT="1")
    finally:
        A.destroy()


# 9. batched, not a loop -------------------------------------------------------------------------------------------------------------------------------
def test_launch_checks_of_a_batch_of_eight_stay_below_five_single_proofs(bench, gpu):
    """a loop -- or lockstep without lane-batched kernels -- passes the launch-check funnel 8x as often as one proof; with lane-batched kernels
    everything but the commitments passes it once, and the commitments need ceil(24/4) + ceil(8/4) + ceil(24/4) + ceil(16/4) = 18 tickets against 4"""
    B = bench(16384)
    ws = [B.witness(j) for j in range(8)]
    B.batch.construct_proofs(ws)  # warm: lanes, tables, workspaces
    B.one(0)
    B.single.set_witness(*B.witness(0))
    s0 = gpu.fault_stats()["launch_checks"]
    B.single.construct_proof()
    s1 = gpu.fault_stats()["launch_checks"]
    B.batch.construct_proofs(ws)
    s2 = gpu.fault_stats()["launch_checks"]
    single, batch = s1 - s0, s2 - s1
    print("launch checks: single proof %d, batch of 8 %d (%.2fx)" % (single, batch, batch / max(single, 1)))
    assert single > 0 and batch < 5 * single, "launch checks of one single proof: %d, of one batch of 8: %d" % (single, batch)


# 10. errors -------------------------------------------------------------------------------------------------------------------------------------------
def test_batch_above_the_size_bound_is_refused(gpu, srs_for):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.plonk import Prover, bench_circuit
    st = bench_circuit(1 << 19, 3, 5).preprocess()
    A = Prover(gpu, st, srs_for(1 << 19))
    try:
        before = gpu.memory_stats()
        with pytest.raises(BbGpuError) as e:
            A.construct_proofs([(st["w_l"], st["w_r"], st["w_o"])] * 9)  # 9 x 2^19 > 2^22
        assert " -2" in str(e.value) or "SIZE" in str(e.value), str(e.value)  # BBGPU_ERR_SIZE
        assert gpu.memory_stats() == before
    finally:
        A.destroy()


FAR = 1 << 62


def _load_golden(name):
    import json
    with open(os.path.join(ROOT, "tests", "golden", name)) as fh:
        return json.load(fh)


def fault_sweep(kind):
    """runs in a process of its own (it ends with bbgpu_shutdown): for k in {0, middle, last} of the times a clean count = 4 batch at 1024 gates passes the
    funnel of `kind`, arm kind:k and run the batch -- an error code, or the right proofs when the library rode it out; nothing stays pending, the next
    batch and the next single proof on the same handle are right; with `alloc` the same over the allocations of a handle's FIRST batch (the lanes)"""
    from barretenberg_amd import BbGpu, BbGpuError
    from barretenberg_amd.plonk import Prover
    G = BbGpu(device=0)
    srs = G.srs_generate(P.mont([SECRET_RAW % FR_MODULUS])[0], 65536)
    B = Bench(G, srs, _load_golden, 1024)
    js = [0, 1, 2, 3]
    ws = [B.witness(j) for j in js]

    def sites_of(run):
        G.fault_inject("%s:%d" % (kind, FAR))
        run()
        st = G.fault_stats()
        G.fault_inject(None)
        return {"alloc": st["alloc_calls"], "h2d": st["h2d_calls"], "d2h": st["d2h_calls"], "launch": st["launch_checks"]}[kind]

    def armed_run(k):
        G.fault_inject("%s:%d" % (kind, k))
        try:
            proofs = B.batch.construct_proofs(ws)
        except BbGpuError as e:
            proofs = None
            print("%s:%d -> %s" % (kind, k, str(e)[:100]))
        st = G.fault_stats()
        assert st["slots_pending"] == 0, (kind, k, st)
        assert st["fired"] == 1 and st["armed"] == 0, (kind, k, st)
        if proofs is not None:  # the library absorbed it
            assert st["absorbed"] >= 1, (kind, k, st)
            B.check(proofs, js)
        G.fault_inject(None)
        B.check(B.batch.construct_proofs(ws), js)  # the next unarmed batch is right

    B.check(B.batch.construct_proofs(ws), js)
    warm = sites_of(lambda: B.check(B.batch.construct_proofs(ws), js))
    print("%s: %d sites in a warm batch" % (kind, warm))
    if kind != "alloc":
        assert warm >= 3, warm  # a warm batch allocates nothing; it uploads, reads back and launches
    for k in sorted({0, warm // 2, warm - 1}) if warm else []:
        armed_run(k)
        assert np.array_equal(B.batch.construct_proof(), B.one(0)[0])  # the single path of the same handle
    if kind == "alloc":
        C0 = Prover(G, B.state, srs)
        cold = sites_of(lambda: C0.construct_proofs(ws))
        C0.destroy()
        print("alloc: %d sites in a handle's first batch" % cold)
        assert cold >= 13, cold  # eleven lane groups, the result slots, the table, the unscaled sigma polynomials
        for k in sorted({0, cold // 2, cold - 1}):
            C1 = Prover(G, B.state, srs)
            live = G.fault_stats()["live_allocations"]
            G.fault_inject("alloc:%d" % k)
            try:
                C1.construct_proofs(ws)
                failed = False
            except BbGpuError:
                failed = True
            st = G.fault_stats()
            G.fault_inject(None)
            assert st["fired"] == 1 and st["slots_pending"] == 0, (k, st)
            if failed and k == 0:
                assert st["live_allocations"] <= live + 1, (k, live, st)  # a refused first allocation leaves no lane behind
            again = C1.construct_proofs(ws)
            for lane, j in enumerate(js):
                assert np.array_equal(again[lane], B.one(j)[0]), (k, lane)
            C1.destroy()
    B.destroy()
    G.srs_release(srs)
    G.shutdown()
    st = G.fault_stats()
    assert st["live_allocations"] == 0 and st["live_bytes"] == 0, st
    print("fault sweep %s ok" % kind)


@pytest.mark.parametrize("kind", ["alloc", "h2d", "d2h", "launch"])
def test_injected_failures_are_reported_and_survived(kind):
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_plonk_batch as t; t.fault_sweep(%r)" % kind], cwd=ROOT, capture_output=True, text=True,
                       timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "fault sweep %s ok" % kind in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# 11. memory -------------------------------------------------------------------------------------------------------------------------------------------
def test_lane_memory_is_counted_and_returned(gpu, srs_for, golden):
    from barretenberg_amd.plonk import Prover
    B = Bench(gpu, srs_for(16384), golden, 16384)
    try:
        ws = [B.witness(j) for j in range(4)]
        B.batch.construct_proofs(ws)  # workspaces, transform scratch and tables are at their size for this call from here on
        C1 = Prover(gpu, B.state, srs_for(16384))
        before = gpu.memory_stats()
        C1.construct_proofs(ws)
        grown = gpu.memory_stats()
        assert grown["staging_bytes"] - before["staging_bytes"] >= 4 * 48 * B.n * 32, (before, grown)
        C1.construct_proofs(ws[:2])  # a smaller batch keeps the lanes
        assert gpu.memory_stats() == grown
        C1.destroy()
        assert gpu.memory_stats() == before
    finally:
        B.destroy()
