"""The batch entry of the resident prover (bbgpu_plonk_construct_proof_batch) on a machine without a GPU: the symbols, the argument checks that
come before the library binds a device, and the premise of the GPU tests' fixtures -- the bench circuit with other witness values is the SAME
circuit (selectors, permutation), so one prover handle serves every lane."""
import ctypes as C

import numpy as np
import pytest

BBGPU_ERR_ARG = -3


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)


def _call(lib, prover, count, wl, wr, wo, out):
    f = lib.lib.bbgpu_plonk_construct_proof_batch
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    rc = f(prover, count, wl, wr, wo, out)
    lib.lib.bbgpu_last_error.restype = C.c_char_p
    return rc, lib.lib.bbgpu_last_error().decode()


def test_batch_entries_exist_and_refuse_bad_arguments_without_a_device(lib):
    from barretenberg_amd.bbgpu import C_ABI_SYMBOLS
    for name in ("bbgpu_plonk_construct_proof_batch", "bbgpu_plonk_batch_challenges", "bbgpu_plonk_last_batch_timing"):
        assert hasattr(lib.lib, name), name
        assert name in C_ABI_SYMBOLS, name
    assert lib.lib.bbgpu_num_contexts() == 1  # (a count, not a binding)
    w = np.zeros((32, 4), dtype=np.uint64)
    col = (C.c_void_p * 17)(*([w.ctypes.data] * 17))
    hole = (C.c_void_p * 17)(*([w.ctypes.data] * 17))
    hole[1] = None
    out = np.zeros((17, 120), dtype=np.uint64)
    cases = [
        ("count", (0, 0, col, col, col, out.ctypes.data)),
        ("count", (0, 17, col, col, col, out.ctypes.data)),
        ("count", (0, -1, col, col, col, out.ctypes.data)),
        ("w_r", (0, 2, col, None, col, out.ctypes.data)),
        ("proofs_out", (0, 2, col, col, col, None)),
        ("w_o[1]", (0, 2, col, col, hole, out.ctypes.data)),
        ("w_l[1]", (0, 3, hole, col, col, out.ctypes.data)),
        ("handle", (0, 2, col, col, col, out.ctypes.data)),       # no prover was ever created
        ("handle", (12345, 1, col, col, col, out.ctypes.data)),
        ("handle", (-1, 1, col, col, col, out.ctypes.data)),
    ]
    for word, args in cases:
        rc, err = _call(lib, *args)
        assert rc == BBGPU_ERR_ARG, (word, args[:2], rc, err)
        assert word in err, (word, err)
    # none of that bound a device: the fault funnels (every allocation, copy and launch check passes one) were never entered
    st = lib.fault_stats()
    assert st["alloc_calls"] == 0 and st["launch_checks"] == 0 and st["h2d_calls"] == 0 and st["live_allocations"] == 0, st
    buf = (C.c_uint64 * 20)()
    lib.lib.bbgpu_plonk_batch_challenges.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    assert lib.lib.bbgpu_plonk_batch_challenges(0, 0, buf) == BBGPU_ERR_ARG
    t = (C.c_double * 4)()
    lib.lib.bbgpu_plonk_last_batch_timing.argtypes = [C.c_int, C.POINTER(C.c_double)]
    assert lib.lib.bbgpu_plonk_last_batch_timing(0, t) == BBGPU_ERR_ARG


CIRCUIT_KEYS = ("sigma_1_mapping", "sigma_2_mapping", "sigma_3_mapping", "q_m", "q_l", "q_r", "q_o", "q_c")


@pytest.mark.parametrize("gates", [32, 1024])
def test_other_witness_values_give_the_same_circuit(golden, gates):
    from barretenberg_amd.plonk import bench_circuit
    tr = golden("plonk_trace.json")
    a0, b0 = int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)
    base = bench_circuit(gates, a0, b0).preprocess()
    for j in (1, 2, 15):
        other = bench_circuit(gates, a0 + j, b0 + 3 * j).preprocess()
        assert other["n"] == base["n"]
        for k in CIRCUIT_KEYS:
            assert np.array_equal(other[k], base[k]), (j, k)
        for k in ("w_l", "w_r", "w_o"):
            assert not np.array_equal(other[k], base[k]), (j, k)


def test_other_mimc_inputs_give_the_same_circuit():
    from barretenberg_amd.plonk import mimc_circuit
    x0, k = 0x0777777788888888555555556666666633333333444444441111111122222222, 0x0ABCDEFABCDEFABC1234123412341234DDDDEEEEFFFF00009999AAAABBBBCCCC
    base = mimc_circuit(30, x0, k).preprocess()
    other = mimc_circuit(30, x0 + 1, k + 5).preprocess()
    for key in CIRCUIT_KEYS + ("q_mimc_selector", "q_mimc_coefficient"):
        assert np.array_equal(other[key], base[key]), key
    assert not np.array_equal(other["w_l"], base["w_l"]) and not np.array_equal(other["w_o"], base["w_o"])
