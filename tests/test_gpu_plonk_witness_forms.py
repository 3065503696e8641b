"""GPU tests (-m gpu) of the witness forms of the resident prover: bbgpu_plonk_prover_set_wire_map, bbgpu_plonk_witness and the three *_from entries
(plonk.hip load_lanes / set_witness_from, poly.hip k_expand_wires_lanes).  A witness may come as expanded wires or as the composer's
variables, from host memory or from device memory handed over from torch.  The bar is the wires path's: whatever the form and the place, every lane's
proof, challenges and check report are byte for byte what set_witness + construct_proof / bbgpu_host_plonk_check_witness give for the expanded wires,
lane 0 equals the reference's golden proof, and the reference's own Verifier accepts a lane.  Witness j of a batch is the circuit built with other
witness values: the same circuit and the same wire map (tests/test_plonk_witness_forms_host.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.pyoracle import FR_MODULUS, PolyOracle as P
from tests import plonk_check_cases as K
from tests import test_gpu_plonk_batch as TB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECRET_RAW = TB.SECRET_RAW
CH = TB.CH
ERR_HIP, ERR_SIZE, ERR_ARG, ERR_STATE, ERR_WITNESS = -1, -2, -3, -4, -6
FUNNELS = ("alloc_calls", "h2d_calls", "d2h_calls", "launch_checks")
KINDS = ("VH", "VD", "WD", "WH")  # variables / wires, host / device
FAR = 1 << 62


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


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


class Forms:
    """one circuit: a handle with the wire map for the new entries, a second one for the wires path (set_witness + construct_proof), witness j in every
    form.  make(j) -> a composer of the circuit with the j-th witness values; or state + (index, variables) for a circuit without a mirror composer."""

    def __init__(self, gpu, srs, make=None, state=None, mapped=None):
        from barretenberg_amd.plonk import Prover
        self.make = make
        if make is not None:
            c0 = make(0)
            state = c0.preprocess()
            *index, v0 = c0.wire_map()
        else:
            index, v0 = mapped
        self.state, self.n, self.index, self.nv, self.srs = state, state["n"], list(index), len(v0), srs
        self._v, self._one = {0: v0}, {}
        for k, key in enumerate(K.WIRES):
            assert np.array_equal(v0[self.index[k]], state[key]), key
        self.A = Prover(gpu, state, srs)
        self.S = Prover(gpu, state, srs)
        self.A.set_wire_map(*self.index, self.nv)

    def variables(self, j):
        if j not in self._v:
            *index, v = self.make(j).wire_map()
            assert all(np.array_equal(a, b) for a, b in zip(index, self.index)) and len(v) == self.nv
            self._v[j] = v
        return self._v[j]

    def wires(self, j):
        v = self.variables(j)
        return tuple(np.ascontiguousarray(v[i]) for i in self.index)

    def item(self, j, kind):
        if kind == "VH":
            return self.variables(j)
        if kind == "VD":
            return on_device(self.variables(j))
        if kind == "WD":
            return tuple(on_device(w) for w in self.wires(j))
        return self.wires(j)

    def one(self, j):
        """(proof, challenges) of witness j from the wires path of the second handle"""
        if j not in self._one:
            self.S.set_witness(*self.wires(j))
            proof = self.S.construct_proof()
            self._one[j] = (proof, {k: v.copy() for k, v in self.S.challenges().items()})
        return self._one[j]

    def check(self, proofs, js, what="", prover=None):
        assert proofs.shape == (len(js), 120)
        for lane, j in enumerate(js):
            want, ch = self.one(j)
            assert np.array_equal(proofs[lane], want), (what, "lane", lane, "witness", j)
            got = (prover or self.A).batch_challenges(lane)
            for name in CH:
                assert np.array_equal(got[name], ch[name]), (what, lane, name)

    def destroy(self):
        self.A.destroy()
        self.S.destroy()


def bench_forms(gpu, srs, golden, gates):
    from barretenberg_amd.plonk import bench_circuit
    tr = golden("plonk_trace.json")
    a0, b0 = int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)
    return Forms(gpu, srs, lambda j: bench_circuit(gates, a0 + j, b0 + 3 * j))


@pytest.fixture(scope="module")
def bench(gpu, srs_for, golden):
    made = {}

    def get(gates):
        if gates not in made:
            made[gates] = bench_forms(gpu, srs_for(gates), golden, gates)
        return made[gates]

    def drop(gates):  # destroyed AND forgotten: a later case of that size builds its own
        made.pop(gates).destroy()
    get.drop = drop
    yield get
    for f in made.values():
        f.destroy()


# 1. bytes ---------------------------------------------------------------------------------------------------------------------------------------------
CASES = [(g, c) for g in (32, 1024, 16384, 65536) for c in (1, 3, 8, 16)] + [(1 << 18, 4), (1 << 20, 2)]


def all_forms(F, js):
    """the batch of witnesses js in each form, and once with the four kinds mixed: every lane is the wires path's proof"""
    out = {}
    for kind in ("VH", "VD", "WD"):
        out[kind] = F.A.construct_proofs_from([F.item(j, kind) for j in js])
        F.check(out[kind], js, kind)
    mixed = F.A.construct_proofs_from([F.item(j, KINDS[lane % 4]) for lane, j in enumerate(js)])
    F.check(mixed, js, "mixed")
    return out


@pytest.mark.parametrize("gates,count", CASES)
def test_proofs_from_every_form_are_byte_identical(bench, golden, gates, count):
    from barretenberg_amd.plonk import proof_lines
    F = bench(gates)
    js = list(range(count))
    out = all_forms(F, js)
    gold = golden("plonk_proofs.json")["proofs"][str(gates)][:26]
    for kind, proofs in out.items():
        assert proof_lines(F.n, proofs[0]) == gold, kind
    if count == 3 and gates <= 65536:  # the reference's Verifier judges a lane of a VARIABLES / DEVICE batch
        TB._verify(proof_lines(F.n, out["VD"][2]), gates)
    if gates > 65536:  # 96 MiB x 4 per lane and handle at 2^18 gates and up: give it back before the next size
        bench.drop(gates)


def _widget(gpu, srs, F, js, gold, **lines_kw):
    from barretenberg_amd.plonk import proof_lines
    try:
        out = all_forms(F, js)
        for kind, proofs in out.items():
            for lane, lines in gold.items():
                assert proof_lines(F.n, proofs[lane], **lines_kw) == lines, (kind, lane)
        return out
    finally:
        F.destroy()


@pytest.mark.parametrize("gates", [6, 64, 4096])
def test_bool_widget_in_every_form(gpu, srs_for, golden, gates):
    from barretenberg_amd.plonk import bool_circuit
    gold = golden("plonk_trace.json")["bool"]["proofs"][str(gates)][:26]
    _widget(gpu, srs_for(65536), Forms(gpu, srs_for(65536), lambda j: bool_circuit(gates)), [0, 0, 0], {0: gold, 2: gold})


@pytest.mark.parametrize("gates", [6, 93, 4094])
def test_mimc_widget_in_every_form(gpu, srs_for, golden, gates):
    from barretenberg_amd.plonk import mimc_circuit
    gold = golden("plonk_trace.json")["mimc"]["proofs"][str(gates)][:28]
    F = Forms(gpu, srs_for(65536), lambda j: mimc_circuit(gates, TB.MIMC_X0 + j, TB.MIMC_K))
    assert not np.array_equal(F.variables(1), F.variables(0))
    _widget(gpu, srs_for(65536), F, [0, 1, 2], {0: gold}, mimc=True)


@pytest.mark.parametrize("gates", [32, 160])
def test_sequential_and_bool_widgets_in_every_form(gpu, srs_for, golden, gates):
    """the extended fixture has no mirror composer: its variable form comes from variables_from_wires"""
    from barretenberg_amd.plonk import variables_from_wires
    st = K.extended_state(gates)
    gold = golden("plonk_trace.json")["extended"]["proofs"][str(gates)][:27]
    F = Forms(gpu, srs_for(65536), state=st, mapped=variables_from_wires(st["w_l"], st["w_r"], st["w_o"]))
    _widget(gpu, srs_for(65536), F, [0, 0, 0], {0: gold, 1: gold, 2: gold}, sequential=True)


def test_commitments_at_infinity_in_every_form(gpu, srs_for):
    from barretenberg_amd.plonk import proof_lines, zero_wire_circuit
    a0 = 0x0777777788888888555555556666666633333333444444441111111122222222
    F = Forms(gpu, srs_for(65536), lambda j: zero_wire_circuit(32, a0 + j))
    try:
        out = all_forms(F, [0, 1, 2])
        for kind, proofs in out.items():
            for lane in range(3):
                got = dict(ln.split() for ln in proof_lines(F.n, proofs[lane])[1:])
                for k in ("W_R", "W_O"):  # the clean encoding of the point at infinity
                    assert got[k + ".x"] == "0" * 64 and got[k + ".y"] == "8" + "0" * 63, (kind, lane, k)
            assert not np.array_equal(proofs[0], proofs[1])
        TB._verify(proof_lines(F.n, out["VD"][1]), 32, BB_CIRCUIT="zerowire", BBGPU_SHIM_STRICT="1")
    finally:
        F.destroy()


def test_uint64_and_cpu_tensors_and_other_streams(bench):
    """a CUDA tensor of dtype uint64 is taken as it is, a CPU tensor goes as host memory, and device data produced on a side stream is ordered behind
    that stream (the copy that fills the tensor is enqueued there, right before the call)"""
    import torch
    F = bench(1024)
    js = [2, 1]
    host = [torch.from_numpy(F.variables(j).view(np.int64)) for j in js]
    F.check(F.A.construct_proofs_from([host[0].view(torch.uint64), host[1]]), js, "cpu tensors")
    F.check(F.A.construct_proofs_from([on_device(F.variables(j)).view(torch.uint64) for j in js]), js, "uint64 on the device")
    side = torch.cuda.Stream()
    pinned = [h.pin_memory() for h in host]
    with torch.cuda.stream(side):
        dev = [torch.empty_like(p, device="cuda") for p in pinned]
        for d, p in zip(dev, pinned):
            d.copy_(p, non_blocking=True)
        proofs = F.A.construct_proofs_from(dev)  # current stream = side
    F.check(proofs, js, "side stream")
    torch.cuda.synchronize()


# 2. the single entry ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gates", [32, 16384])
def test_set_variables_equals_set_witness(bench, gpu, gates):
    F = bench(gates)
    for j, kind in ((1, "VH"), (2, "VD"), (3, "WD"), (0, "VH")):
        if kind == "WD":
            F.A.set_witness_from(F.item(j, kind))
        else:
            F.A.set_variables(F.item(j, kind))
        want, ch = F.one(j)
        assert np.array_equal(F.A.construct_proof(), want), (j, kind)
        got = F.A.challenges()
        for name in CH:
            assert np.array_equal(got[name], ch[name]), (j, kind, name)
        F.S.set_witness(*F.wires(j))
        assert F.A.check_witness() == F.S.check_witness() and K.is_clear(F.A.check_witness())
    # a corrupted variable: the report of the expanded wires
    v = F.variables(1).copy()
    v[F.index[2][F.n // 3]] = K.mont(12345)
    wires = tuple(np.ascontiguousarray(v[i]) for i in F.index)
    F.A.set_variables(on_device(v))
    F.S.set_witness(*wires)
    got = F.A.check_witness()
    assert got == F.S.check_witness() and not K.is_clear(got)
    from barretenberg_amd.plonk import host_check_witness
    want = host_check_witness(dict(F.state, w_l=wires[0], w_r=wires[1], w_o=wires[2]), gpu)
    assert {k: got[k] for k in K.FIELDS} == {k: want[k] for k in K.FIELDS}
    F.A.set_variables(F.variables(0))


# 3. the check -----------------------------------------------------------------------------------------------------------------------------------------
def _variable_form(index, variables, honest, state):
    """the perturbed witness of a case as variables: every cell that differs from the honest witness corrupts the variable it maps to.
    -> (variables, the state those variables expand to)"""
    v = variables.copy()
    for k, key in enumerate(K.WIRES):
        rows = np.nonzero((np.asarray(state[key]) != np.asarray(honest[key])).any(axis=1))[0]
        v[index[k][rows]] = np.asarray(state[key])[rows]
    expanded = dict(state)
    for k, key in enumerate(K.WIRES):
        expanded[key] = np.ascontiguousarray(v[index[k]])
    return v, expanded


@pytest.mark.parametrize("name", K.ALL_CIRCUITS)
def test_check_reports_of_variable_forms_equal_the_host_entry(gpu, srs_for, name):
    from barretenberg_amd.plonk import Prover, host_check_witness, variables_from_wires
    state = K.circuit(name)
    cases = K.cases(name, state)
    index, variables = variables_from_wires(*(state[k] for k in K.WIRES))
    own = [c for c in cases if not c.circuit_changed]
    forms = [_variable_form(index, variables, state, c.state) for c in own]
    want = [host_check_witness(st, gpu) for _, st in forms]
    assert K.is_clear(want[0]) and any(not K.is_clear(w) for w in want), [c.name for c in own]
    A = Prover(gpu, state, srs_for(state["n"]))
    try:
        A.set_wire_map(*index, len(variables))
        for lo in range(0, len(forms), 16):
            part = forms[lo:lo + 16]
            for place in (lambda v: v, on_device):
                got = A.check_witnesses_from([place(v) for v, _ in part])
                for lane, rep in enumerate(got):
                    w = want[lo + lane]
                    print(name, own[lo + lane].name, rep)
                    assert {k: rep[k] for k in K.FIELDS} == {k: w[k] for k in K.FIELDS}, (name, own[lo + lane].name, rep, w)
                    assert A.last_witness_report(lane) == rep
            mixed = A.check_witnesses_from([v if lane % 2 else tuple(on_device(st[k]) for k in K.WIRES) for lane, (v, st) in enumerate(part)])
            assert mixed == got
    finally:
        A.destroy()
    for c in cases:
        if c.circuit_changed:  # a redirected mapping entry is another circuit: a handle of its own, the honest variables
            B = Prover(gpu, c.state, srs_for(state["n"]))
            try:
                B.set_wire_map(*index, len(variables))
                w = host_check_witness(c.state, gpu)
                got = B.check_witnesses_from([variables, on_device(variables)])
                for rep in got:
                    assert {k: rep[k] for k in K.FIELDS} == {k: w[k] for k in K.FIELDS}, (name, c.name, rep, w)
            finally:
                B.destroy()


def test_checked_batch_of_variables_raises_and_writes_nothing(bench, gpu):
    from barretenberg_amd.bbgpu import PlonkWitness
    from barretenberg_amd.plonk import WitnessError
    F = bench(1024)
    bad = F.variables(1).copy()
    bad[F.index[2][F.n // 3]] = K.mont(777)
    items = [F.variables(0), on_device(bad), F.variables(2)]
    F.A.set_witness_check(True)
    try:
        with pytest.raises(WitnessError) as e:
            F.A.construct_proofs_from(items)
        assert e.value.bad_lanes() == [1] and "lane 1" in str(e.value)
        descs, keep = F.A._describe_all(items)
        out = np.full((3, 120), 0xABABABABABABABAB, dtype=np.uint64)
        f = gpu.lib.bbgpu_plonk_construct_proof_batch_from
        f.argtypes = [C.c_int, C.c_int, C.POINTER(PlonkWitness), C.c_void_p]
        assert f(F.A.handle, 3, descs, out.ctypes.data) == ERR_WITNESS
        assert (out == 0xABABABABABABABAB).all(), "no proof bytes of any lane"
        assert gpu.fault_stats()["slots_pending"] == 0
        del keep
        F.check(F.A.construct_proofs_from([F.variables(0), F.variables(2)]), [0, 2], "checked, all good")
    finally:
        F.A.set_witness_check(False)
    F.check(F.A.construct_proofs_from(items[:1]), [0])


# 4. funnels -------------------------------------------------------------------------------------------------------------------------------------------
def test_funnel_counts_of_the_forms(bench, gpu):
    """one copy per lane instead of three (none from device memory), one more launch (the expansion) and one more copy (its record table) per batch"""
    F = bench(16384)
    count = 8
    js = list(range(count))
    items = {kind: [F.item(j, kind) for j in js] for kind in KINDS}
    for kind in KINDS:
        F.A.construct_proofs_from(items[kind])  # warm: lanes, staging, tables, workspaces

    def funnels(run):
        s0 = gpu.fault_stats()
        run()
        s1 = gpu.fault_stats()
        return {k: s1[k] - s0[k] for k in FUNNELS}

    old = funnels(lambda: F.A.construct_proofs(items["WH"]))
    wires = funnels(lambda: F.A.construct_proofs_from(items["WH"]))
    vh = funnels(lambda: F.A.construct_proofs_from(items["VH"]))
    vd = funnels(lambda: F.A.construct_proofs_from(items["VD"]))
    print("construct_proofs %s\nWIRES/HOST %s\nVARIABLES/HOST %s\nVARIABLES/DEVICE %s" % (old, wires, vh, vd))
    assert wires == old, "WIRES / HOST is the path of construct_proofs, funnel for funnel"
    assert vh["h2d_calls"] <= wires["h2d_calls"] - 2 * count + 1 and vh["launch_checks"] <= wires["launch_checks"] + 1, (vh, wires)
    assert vd["h2d_calls"] <= wires["h2d_calls"] - 3 * count + 1 and vd["launch_checks"] <= wires["launch_checks"] + 1, (vd, wires)
    assert old["alloc_calls"] == vh["alloc_calls"] == vd["alloc_calls"] == 0
    # the check entry fills the lanes (and their variables staging) a proof of the same count uses: that proof allocates nothing
    from barretenberg_amd.plonk import Prover
    # (what a handle's first proof batch still allocates after a check is its scan / evaluation scratch: the same with wires and with variables)
    B, Bw = Prover(gpu, F.state, F.srs), Prover(gpu, F.state, F.srs)
    try:
        B.set_wire_map(*F.index, F.nv)
        assert all(K.is_clear(r) for r in B.check_witnesses_from(items["VH"]))
        assert all(K.is_clear(r) for r in Bw.check_witnesses(items["WH"]))
        first = funnels(lambda: F.check(B.construct_proofs_from(items["VH"]), js, "after a check", B))
        first_wires = funnels(lambda: F.check(Bw.construct_proofs(items["WH"]), js, "after a check, wires", Bw))
        second = funnels(lambda: F.check(B.construct_proofs_from(items["VH"]), js, "second batch", B))
        print("after a check: first batch %s (wires %s), second batch %s" % (first, first_wires, second))
        assert first["alloc_calls"] == first_wires["alloc_calls"] and second["alloc_calls"] == 0, (first, first_wires, second)
        old_check = funnels(lambda: B.check_witnesses(items["WH"]))
        new_check = funnels(lambda: B.check_witnesses_from(items["WH"]))
        assert old_check == new_check
    finally:
        B.destroy()
        Bw.destroy()


# 5. refusals that touch the runtime -------------------------------------------------------------------------------------------------------------------
def _raw(gpu):
    from barretenberg_amd.bbgpu import PlonkWitness, WitnessReport
    L = gpu.lib
    L.bbgpu_plonk_prover_set_wire_map.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.bbgpu_plonk_prover_set_witness_from.argtypes = [C.c_int, C.POINTER(PlonkWitness)]
    L.bbgpu_plonk_construct_proof_batch_from.argtypes = [C.c_int, C.c_int, C.POINTER(PlonkWitness), C.c_void_p]
    L.bbgpu_plonk_check_witness_batch_from.argtypes = [C.c_int, C.c_int, C.POINTER(PlonkWitness), C.POINTER(WitnessReport)]
    return L, PlonkWitness, WitnessReport


def test_device_descriptors_that_are_not_device_memory_are_refused(bench, gpu):
    """pinned host memory on purpose: were the validation missing, the kernel would read GPU-mapped memory and this test would fail on the return code;
    the card would not fault"""
    import torch
    L, PlonkWitness, WitnessReport = _raw(gpu)
    F = bench(1024)
    pinned = torch.from_numpy(F.variables(0).view(np.int64)).pin_memory()
    pinned_w = [torch.from_numpy(w.view(np.int64)).pin_memory() for w in F.wires(0)]
    dev = on_device(np.concatenate([F.variables(0), F.variables(0)[:1]]))
    out = np.zeros((2, 120), dtype=np.uint64)
    reps = (WitnessReport * 2)()

    def variables_at(ptr):
        d = PlonkWitness()
        d.form, d.where, d.variables = PlonkWitness.VARIABLES, PlonkWitness.DEVICE, ptr
        return d

    wires = PlonkWitness()
    wires.form, wires.where = PlonkWitness.WIRES, PlonkWitness.DEVICE
    dev_l = on_device(F.wires(0)[0])
    wires.w_l, wires.w_r, wires.w_o = dev_l.data_ptr(), pinned_w[1].data_ptr(), pinned_w[2].data_ptr()
    good = variables_at(dev.data_ptr())
    before = gpu.fault_stats()
    for word, d in (("host memory", variables_at(pinned.data_ptr())), ("w_r", wires), ("aligned", variables_at(dev.data_ptr() + 8))):
        for call in (lambda: L.bbgpu_plonk_prover_set_witness_from(F.A.handle, C.byref(d)),
                     lambda: L.bbgpu_plonk_construct_proof_batch_from(F.A.handle, 2, (PlonkWitness * 2)(good, d), out.ctypes.data),
                     lambda: L.bbgpu_plonk_check_witness_batch_from(F.A.handle, 2, (PlonkWitness * 2)(good, d), reps)):
            rc = call()
            err = L.bbgpu_last_error().decode()
            assert rc == ERR_ARG and word in err, (word, rc, err)
    after = gpu.fault_stats()
    assert {k: after[k] for k in FUNNELS} == {k: before[k] for k in FUNNELS}, (before, after)  # nothing was allocated, copied or launched
    assert not out.any()
    F.check(F.A.construct_proofs_from([dev[:F.nv], F.variables(1)]), [0, 1], "after the refusals")


def test_wire_map_checks_that_need_the_circuit_size(gpu, srs_for, golden):
    """an index >= num_variables, num_variables > 4 n: refused on the host, before anything is allocated, copied or launched; and VARIABLES without a map"""
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.plonk import Prover
    L, PlonkWitness, WitnessReport = _raw(gpu)
    F = bench_forms(gpu, srs_for(1024), golden, 1024)
    B = Prover(gpu, F.state, srs_for(1024))
    try:
        n = F.n
        idx = [a.copy() for a in F.index]
        bad = idx[1].copy()
        bad[77] = F.nv
        bad[500] = F.nv + 9
        last = idx[2].copy()
        last[n - 1] = 0xFFFFFFFF
        before = gpu.fault_stats()
        for code, word, args in ((ERR_ARG, "w_r_index[77]", (idx[0], bad, idx[2], F.nv)), (ERR_ARG, "w_o_index[%d]" % (n - 1), (idx[0], idx[1], last, F.nv)),
                                 (ERR_SIZE, "num_variables", (idx[0], idx[1], idx[2], 4 * n + 1)), (ERR_SIZE, "num_variables", (idx[0], idx[1], idx[2], 0))):
            rc = L.bbgpu_plonk_prover_set_wire_map(B.handle, args[0].ctypes.data, args[1].ctypes.data, args[2].ctypes.data, args[3])
            err = L.bbgpu_last_error().decode()
            assert rc == code and word in err, (word, rc, err)
        # no map yet: the VARIABLES form is a state error, from every entry and place
        d = PlonkWitness()
        d.form, d.where, d.variables = PlonkWitness.VARIABLES, PlonkWitness.HOST, F.variables(0).ctypes.data
        out = np.zeros((1, 120), dtype=np.uint64)
        reps = (WitnessReport * 1)()
        assert L.bbgpu_plonk_prover_set_witness_from(B.handle, C.byref(d)) == ERR_STATE and "wire map" in L.bbgpu_last_error().decode()
        assert L.bbgpu_plonk_construct_proof_batch_from(B.handle, 1, C.byref(d), out.ctypes.data) == ERR_STATE
        assert L.bbgpu_plonk_check_witness_batch_from(B.handle, 1, C.byref(d), reps) == ERR_STATE
        after = gpu.fault_stats()
        assert {k: after[k] for k in FUNNELS} == {k: before[k] for k in FUNNELS}, (before, after)
        with pytest.raises(BbGpuError):
            B.construct_proofs_from([on_device(F.variables(0))])
        # num_variables == 4 n is allowed (variables no gate uses), and a second map replaces the first
        B.set_wire_map(*F.index, 4 * n)
        padded = np.zeros((4 * n, 4), dtype=np.uint64)
        padded[:F.nv] = F.variables(1)
        assert np.array_equal(B.construct_proofs_from([padded, on_device(padded)])[1], F.one(1)[0])
        B.set_wire_map(*F.index, F.nv)
        assert np.array_equal(B.construct_proofs_from([F.variables(2)])[0], F.one(2)[0])
        B.set_variables(F.variables(1))
        assert np.array_equal(B.construct_proof(), F.one(1)[0])
    finally:
        B.destroy()
        F.destroy()


# 6. memory --------------------------------------------------------------------------------------------------------------------------------------------
def test_map_and_staging_are_counted_and_returned(gpu, srs_for, golden):
    from barretenberg_amd.plonk import Prover
    F = bench_forms(gpu, srs_for(16384), golden, 16384)
    try:
        items = [F.variables(j) for j in range(4)]
        F.A.construct_proofs_from(items)  # workspaces, transform scratch and tables are at their size for this call from here on
        F.A.set_variables(items[0])
        before = gpu.memory_stats()
        C1 = Prover(gpu, F.state, srs_for(16384))
        created = gpu.memory_stats()
        C1.set_wire_map(*F.index, F.nv)
        mapped = gpu.memory_stats()
        assert mapped["staging_bytes"] - created["staging_bytes"] == 3 * F.n * 4, (created, mapped)
        C1.set_variables(items[1])
        staged = gpu.memory_stats()
        assert staged["staging_bytes"] - mapped["staging_bytes"] == F.nv * 32, (mapped, staged)
        C1.set_variables(on_device(items[1]))  # device variables are read where they are
        assert gpu.memory_stats() == staged
        C1.check_witnesses_from(items)
        C1.construct_proofs_from(items)
        grown = gpu.memory_stats()
        assert grown["staging_bytes"] - staged["staging_bytes"] >= 4 * (48 * F.n + F.nv) * 32, (staged, grown)
        C1.construct_proofs_from(items[:2])  # a smaller batch keeps the lanes and their variables
        C1.check_witnesses_from(items[:3])
        assert gpu.memory_stats() == grown
        C1.destroy()
        assert gpu.memory_stats() == before
    finally:
        F.destroy()


# 7. injected failures ---------------------------------------------------------------------------------------------------------------------------------
def fault_sweep(kind):
    """runs in a process of its own (it ends with bbgpu_shutdown): over EVERY site k of `kind` that one cold VARIABLES / HOST batch of 3 lanes at 1024 gates
    passes -- a fresh handle each time: its map is set, then kind:k is armed and the batch runs -- the call returns an error code, or the right proofs when
    the library rode the failure out; nothing stays pending; the next unarmed call on the same handle returns the right bytes"""
    from barretenberg_amd import BbGpu, BbGpuError
    from barretenberg_amd.plonk import Prover
    G = BbGpu(device=0)
    srs = G.srs_generate(P.mont([SECRET_RAW % FR_MODULUS])[0], 65536)
    F = bench_forms(G, srs, TB._load_golden, 1024)
    js = [0, 1, 2]
    items = [F.variables(j) for j in js]
    want = [F.one(j)[0] for j in js]

    def fresh():
        p = Prover(G, F.state, srs)
        p.set_wire_map(*F.index, F.nv)
        return p

    def right(proofs):
        return all(np.array_equal(proofs[lane], want[lane]) for lane in range(3))

    W = fresh()
    assert right(W.construct_proofs_from(items))  # the library's own workspaces and tables are warm from here on; every handle below is cold
    W.destroy()
    C0 = fresh()
    G.fault_inject("%s:%d" % (kind, FAR))
    assert right(C0.construct_proofs_from(items))
    st = G.fault_stats()
    G.fault_inject(None)
    C0.destroy()
    sites = {"alloc": st["alloc_calls"], "h2d": st["h2d_calls"], "launch": st["launch_checks"]}[kind]
    print("%s: %d sites in a cold batch" % (kind, sites))
    assert sites >= {"alloc": 14, "h2d": 4, "launch": 20}[kind], sites  # (alloc: the lane groups, the slots, the table, sigma, the variables group)
    failed = absorbed = 0
    for k in range(sites):
        C1 = fresh()
        G.fault_inject("%s:%d" % (kind, k))
        try:
            proofs = C1.construct_proofs_from(items)
        except BbGpuError as e:
            proofs = None
            failed += 1
            assert int(str(e).split()[2].rstrip(":")) == ERR_HIP, (kind, k, str(e))
        st = G.fault_stats()
        G.fault_inject(None)
        assert st["fired"] == 1 and st["armed"] == 0 and st["slots_pending"] == 0, (kind, k, st)
        if proofs is not None:
            assert st["absorbed"] >= 1 and right(proofs), (kind, k, st)
            absorbed += 1
        assert right(C1.construct_proofs_from(items)), (kind, k)  # the next clean call
        assert G.fault_stats()["slots_pending"] == 0
        C1.destroy()
    print("%s: %d failed, %d absorbed" % (kind, failed, absorbed))
    assert failed > 0
    F.destroy()
    G.srs_release(srs)
    G.shutdown()
    st = G.fault_stats()
    assert st["live_allocations"] == 0 and st["live_bytes"] == 0, st
    print("fault sweep %s ok" % kind)


@pytest.mark.parametrize("kind", ["alloc", "h2d", "launch"])
def test_injected_failures_are_reported_and_survived(kind):
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_plonk_witness_forms as t; t.fault_sweep(%r)" % kind], cwd=ROOT, capture_output=True,
                       text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "fault sweep %s ok" % kind in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
