"""Witnesses as composer variables, from host or device memory (bbgpu_plonk_prover_set_wire_map, bbgpu_plonk_witness and the three *_from entries) on a
machine without a GPU: the symbols, the argument checks that come before the library binds a device, and the premise of the GPU tests -- a composer's
wire_map() expands to exactly the wires its preprocess() returns, the map is a property of the circuit, and variables_from_wires gives any expanded
witness a variable form.

What of the argument checks can run here: a prover handle exists only on a machine with a GPU, and the two checks of bbgpu_plonk_prover_set_wire_map
that need the circuit size n (an index >= num_variables names a ROW of an n-entry array, num_variables > 4 n) come after the handle lookup.  They are
tested on a created prover in tests/test_gpu_plonk_witness_forms.py, with the same "no allocation, copy or launch check afterwards" assertion; every
check that does not need n is tested here."""
import ctypes as C

import numpy as np
import pytest

BBGPU_ERR_SIZE, BBGPU_ERR_ARG = -2, -3
NEW_SYMBOLS = ("bbgpu_plonk_prover_set_wire_map", "bbgpu_plonk_prover_set_witness_from", "bbgpu_plonk_construct_proof_batch_from",
               "bbgpu_plonk_check_witness_batch_from")
MIMC_X0 = 0x0777777788888888555555556666666633333333444444441111111122222222
MIMC_K = 0x0ABCDEFABCDEFABC1234123412341234DDDDEEEEFFFF00009999AAAABBBBCCCC


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)


def test_the_four_symbols_exist_everywhere(lib):
    import os
    import re
    from barretenberg_amd.bbgpu import C_ABI_SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bbgpu.h")).read()
    declared = set(re.findall(r"\b(bbgpu_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_SYMBOLS:
        assert hasattr(lib.lib, name), name
        assert name in declared, name
        assert name in C_ABI_SYMBOLS, name
    for word in ("BBGPU_PLONK_WITNESS_WIRES = 0", "BBGPU_PLONK_WITNESS_VARIABLES = 1", "BBGPU_PLONK_WITNESS_HOST = 0", "BBGPU_PLONK_WITNESS_DEVICE = 1",
                 "} bbgpu_plonk_witness;", "standard_composer.cpp:205-209"):
        assert word in hdr, word


def _err(lib):
    lib.lib.bbgpu_last_error.restype = C.c_char_p
    return lib.lib.bbgpu_last_error().decode()


def test_bad_arguments_are_refused_without_a_device(lib):
    from barretenberg_amd.bbgpu import PlonkWitness, WitnessReport
    L = lib.lib
    L.bbgpu_plonk_prover_set_wire_map.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.bbgpu_plonk_prover_set_witness_from.argtypes = [C.c_int, C.POINTER(PlonkWitness)]
    L.bbgpu_plonk_construct_proof_batch_from.argtypes = [C.c_int, C.c_int, C.POINTER(PlonkWitness), C.c_void_p]
    L.bbgpu_plonk_check_witness_batch_from.argtypes = [C.c_int, C.c_int, C.POINTER(PlonkWitness), C.POINTER(WitnessReport)]
    assert C.sizeof(PlonkWitness) == 48  # two ints, five pointers: the layout of the header's struct
    w = np.zeros((32, 4), dtype=np.uint64)
    idx = np.zeros(32, dtype=np.uint32)
    out = np.zeros((17, 120), dtype=np.uint64)
    reps = (WitnessReport * 17)()

    def desc(form=0, where=0, w_l=w, w_r=w, w_o=w, variables=w):
        d = PlonkWitness()
        d.form, d.where = form, where
        for k, a in (("w_l", w_l), ("w_r", w_r), ("w_o", w_o), ("variables", variables)):
            setattr(d, k, None if a is None else a.ctypes.data)
        return d

    def arr(*ds):
        return (PlonkWitness * 17)(*ds)

    good = desc()
    p = idx.ctypes.data
    cases = [
        # the wire map
        (BBGPU_ERR_ARG, "w_l_index", lambda: L.bbgpu_plonk_prover_set_wire_map(0, None, p, p, 8)),
        (BBGPU_ERR_ARG, "w_r_index", lambda: L.bbgpu_plonk_prover_set_wire_map(0, p, None, p, 8)),
        (BBGPU_ERR_ARG, "w_o_index", lambda: L.bbgpu_plonk_prover_set_wire_map(0, p, p, None, 8)),
        (BBGPU_ERR_SIZE, "num_variables", lambda: L.bbgpu_plonk_prover_set_wire_map(0, p, p, p, 0)),
        (BBGPU_ERR_ARG, "handle", lambda: L.bbgpu_plonk_prover_set_wire_map(0, p, p, p, 8)),  # no prover was ever created
        # the single entry
        (BBGPU_ERR_ARG, "descriptor", lambda: L.bbgpu_plonk_prover_set_witness_from(0, None)),
        (BBGPU_ERR_ARG, "form", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(desc(form=2)))),
        (BBGPU_ERR_ARG, "form", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(desc(form=-1)))),
        (BBGPU_ERR_ARG, "where", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(desc(where=2)))),
        (BBGPU_ERR_ARG, "w_r", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(desc(w_r=None)))),
        (BBGPU_ERR_ARG, "variables", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(desc(form=1, variables=None)))),
        (BBGPU_ERR_ARG, "variables", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(desc(form=1, where=1, variables=None)))),
        (BBGPU_ERR_ARG, "handle", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(good))),
        (BBGPU_ERR_ARG, "handle", lambda: L.bbgpu_plonk_prover_set_witness_from(0, C.byref(desc(form=1, w_l=None, w_r=None, w_o=None)))),  # VARIABLES needs no wires
        # the batch entries
        (BBGPU_ERR_ARG, "count", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 0, arr(good), out.ctypes.data)),
        (BBGPU_ERR_ARG, "count", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 17, arr(*[good] * 17), out.ctypes.data)),
        (BBGPU_ERR_ARG, "count", lambda: L.bbgpu_plonk_check_witness_batch_from(0, -1, arr(good), reps)),
        (BBGPU_ERR_ARG, "descriptors", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 2, None, out.ctypes.data)),
        (BBGPU_ERR_ARG, "descriptors", lambda: L.bbgpu_plonk_check_witness_batch_from(0, 2, None, reps)),
        (BBGPU_ERR_ARG, "proofs_out", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 2, arr(good, good), None)),
        (BBGPU_ERR_ARG, "out", lambda: L.bbgpu_plonk_check_witness_batch_from(0, 2, arr(good, good), None)),
        (BBGPU_ERR_ARG, "witness[1]: unknown form", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 2, arr(good, desc(form=7)), out.ctypes.data)),
        (BBGPU_ERR_ARG, "witness[2]: unknown where", lambda: L.bbgpu_plonk_check_witness_batch_from(0, 3, arr(good, good, desc(where=-3)), reps)),
        (BBGPU_ERR_ARG, "witness[1]: null pointer: w_o", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 2, arr(good, desc(w_o=None)), out.ctypes.data)),
        (BBGPU_ERR_ARG, "witness[0]: null pointer: variables", lambda: L.bbgpu_plonk_check_witness_batch_from(0, 1, arr(desc(form=1, variables=None)), reps)),
        (BBGPU_ERR_ARG, "witness[1]: null pointer: w_l", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 2, arr(good, desc(where=1, w_l=None)), out.ctypes.data)),
        (BBGPU_ERR_ARG, "handle", lambda: L.bbgpu_plonk_construct_proof_batch_from(0, 2, arr(good, desc(form=1)), out.ctypes.data)),
        (BBGPU_ERR_ARG, "handle", lambda: L.bbgpu_plonk_check_witness_batch_from(12345, 1, arr(good), reps)),
        (BBGPU_ERR_ARG, "handle", lambda: L.bbgpu_plonk_construct_proof_batch_from(-1, 1, arr(good), out.ctypes.data)),
    ]
    for code, word, call in cases:
        rc = call()
        err = _err(lib)
        assert rc == code, (word, rc, err)
        assert word in err, (word, err)
    assert not out.any()
    # none of that bound a device: the fault funnels (every allocation, copy and launch check passes one) were never entered
    st = lib.fault_stats()
    assert st["alloc_calls"] == 0 and st["launch_checks"] == 0 and st["h2d_calls"] == 0 and st["live_allocations"] == 0, st


def _circuits(golden):
    from barretenberg_amd.plonk import bench_circuit, bool_circuit, mimc_circuit, zero_wire_circuit
    tr = golden("plonk_trace.json")
    a0, b0 = int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)
    return {
        "bench_32": lambda j: bench_circuit(32, a0 + j, b0 + 3 * j),
        "bench_1024": lambda j: bench_circuit(1024, a0 + j, b0 + 3 * j),
        "bool_64": lambda j: bool_circuit(64),
        "mimc_30": lambda j: mimc_circuit(30, MIMC_X0 + j, MIMC_K + 5 * j),
        "mimc_93": lambda j: mimc_circuit(93, MIMC_X0 + j, MIMC_K),
        "zero_wire_32": lambda j: zero_wire_circuit(32, MIMC_X0 + j),
    }


@pytest.mark.parametrize("name", ["bench_32", "bench_1024", "bool_64", "mimc_30", "mimc_93", "zero_wire_32"])
def test_wire_map_expands_to_the_wires_of_preprocess(golden, name):
    from barretenberg_amd.plonk import variables_from_wires
    make = _circuits(golden)[name]
    composer = make(0)
    state = composer.preprocess()
    n = state["n"]
    *index, variables = composer.wire_map()
    assert variables.dtype == np.uint64 and variables.shape[1] == 4 and 0 < len(variables) <= 4 * n  # the bound of bbgpu_plonk_prover_set_wire_map
    for k, key in enumerate(("w_l", "w_r", "w_o")):
        assert index[k].dtype == np.uint32 and index[k].shape == (n,) and int(index[k].max()) < len(variables), key
        assert np.array_equal(variables[index[k]], state[key]), key  # limb for limb
    # wire_map() before preprocess() (the MiMC composer closes its chain in either): the same map, the same state
    fresh = make(0)
    *index2, variables2 = fresh.wire_map()
    state2 = fresh.preprocess()
    assert all(np.array_equal(a, b) for a, b in zip(index, index2)) and np.array_equal(variables, variables2)
    assert all(np.array_equal(state[k], state2[k]) for k in state if k != "n")
    # other witness values: the same map, other variables
    for j in (1, 2, 15):
        other = make(j)
        *oindex, ovariables = other.wire_map()
        for k in range(3):
            assert np.array_equal(oindex[k], index[k]), (j, k)
        ostate = other.preprocess()
        for k, key in enumerate(("w_l", "w_r", "w_o")):
            assert np.array_equal(ovariables[index[k]], ostate[key]), (j, key)
        if not name.startswith("bool"):
            assert not np.array_equal(ovariables, variables), j
    # any expanded witness has a variable form
    idx, var = variables_from_wires(state["w_l"], state["w_r"], state["w_o"])
    assert var.dtype == np.uint64 and len(var) <= len(variables)
    for k, key in enumerate(("w_l", "w_r", "w_o")):
        assert idx[k].dtype == np.uint32 and np.array_equal(var[idx[k]], state[key]), key


@pytest.mark.parametrize("gates", [32, 160])
def test_variables_from_wires_serves_a_state_without_a_composer(gates):
    from barretenberg_amd.plonk import variables_from_wires
    from tests.plonk_check_cases import extended_state, other_representatives
    st = extended_state(gates)
    for state in (st, other_representatives(st)):  # rows are told apart bit for bit: representatives of one residue are two variables
        idx, var = variables_from_wires(state["w_l"], state["w_r"], state["w_o"])
        assert len(var) <= 3 * st["n"]
        for k, key in enumerate(("w_l", "w_r", "w_o")):
            assert np.array_equal(var[idx[k]], state[key]), key
