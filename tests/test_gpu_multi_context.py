"""GPU tests (-m gpu) of several device contexts in one process (bbgpu_init_devices): the host-pointer MSMs split over N contexts on device 0
against the reference's points and against the one-context answer, the memory each context holds, everything else staying on context 0, the
error contract, and the shim driven by the reference's calling pattern.  Every fixture that binds contexts shuts them down again, so the modules
after this one find the library unbound."""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FR_MODULUS, NTT_KINDS, aligned_copy
from tests.util import CONST_SEED, NTT_SEED, SCALAR_SEED, limbs, noncanonical, sha

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_N = 1 << 17  # two slices of 2^16 points whatever N >= 2 is


def _check(out, case):
    if "infinity" in case:
        assert bool(int(out[7]) >> 63) == case["infinity"]
    else:
        assert np.array_equal(out[0:4], limbs(case["x"])) and np.array_equal(out[4:8], limbs(case["y"])), case
        assert not (int(out[7]) >> 63)


def _neg(scalars):
    rows = [(FR_MODULUS - int.from_bytes(r.tobytes(), "little")) % FR_MODULUS for r in scalars]
    return aligned_copy(np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in rows], dtype=np.uint64))


@pytest.fixture(scope="module")
def tables(golden):
    """the 2^20-point synthetic SRS of msm.json (host endo table), its scalars, and the inputs of the cross-slice edge cases"""
    from barretenberg_amd import BbGpu
    from oracle.pyoracle import Oracle
    g = golden("msm.json")
    n = 1 << 20
    gpu = BbGpu(device=0)
    try:
        _, table = gpu.srs_generate(limbs(g["srs_secret_mont"]), n, want_host_table=True)
    finally:
        gpu.shutdown()
    assert sha(table[0::2]) == g["srs_digest_1048576"]
    scalars = Oracle().random_scalars(SCALAR_SEED, n)
    half = EDGE_N // 2
    rep = aligned_copy(np.concatenate([table[:2 * half], table[:2 * half]]))  # the second half of the table repeats the first
    s = scalars[:half]
    edge = {
        "equal": aligned_copy(np.concatenate([s, s])),                              # equal partial sums: a doubling in the fold
        "opposite": aligned_copy(np.concatenate([s, _neg(s)])),                     # opposite partial sums: the point at infinity
        "zero_slice": aligned_copy(np.concatenate([s, np.zeros_like(s)])),          # the second slice's scalars all zero
    }
    return g, table, scalars, rep, edge


@pytest.fixture(scope="module")
def one_context(tables):
    """the one-context answers for the edge inputs (the same library, bound to one context, before any test binds several)"""
    from barretenberg_amd import BbGpu
    g, table, scalars, rep, edge = tables
    gpu = BbGpu(device=0)
    try:
        single = {k: gpu.pippenger(v, aligned_copy(rep), EDGE_N) for k, v in edge.items()}
        single["batch"] = gpu.batched_scalar_multiplications([(aligned_copy(rep), v, EDGE_N) for v in edge.values()])
        assert gpu.num_contexts() == 1
    finally:
        gpu.shutdown()
    return single


@pytest.fixture(scope="module", params=[2, 3, 8])
def mc(request, one_context):
    from barretenberg_amd import BbGpu
    gpu = BbGpu(devices=[0] * request.param)
    gpu.N = request.param
    try:
        assert gpu.num_contexts() == request.param
        yield gpu
    finally:
        gpu.shutdown()


def test_msm_2_20_against_the_reference(mc, tables):
    """msm.json's 2^20 case: through pippenger (a table registered on first sight: sliced over every context) and through
    batched_scalar_multiplications (3 jobs: each context takes its slice of every job)"""
    g, table, scalars, _, _ = tables
    n = 1 << 20
    case = [c for c in g["cases"] if c["n"] == n][0]
    t = aligned_copy(table)
    _check(mc.pippenger(scalars, t, n), case)
    _check(mc.pippenger(scalars, t, n), case)  # every slice resident now
    rev = aligned_copy(scalars[::-1])
    outs = mc.batched_scalar_multiplications([(t, scalars, n), (t, rev, n), (t, scalars, n)])
    _check(outs[0], case)
    _check(outs[2], case)
    assert np.array_equal(outs[1], mc.pippenger(rev, t, n))
    assert mc.fault_stats()["slots_pending"] == 0


def test_msm_below_the_split(mc, oracle, golden):
    """batched_3x4096: below 2^17 points context 0 runs the call alone"""
    g = golden("msm.json")
    n = 1 << 16
    srs = oracle.make_srs(limbs(g["srs_secret_mont"]), n)
    table = oracle.point_table(srs)
    big = oracle.random_scalars(SCALAR_SEED, 3 * 4096)
    before = [mc.memory_stats(k)["srs_points_bytes"] for k in range(1, mc.N)]
    outs = mc.batched_scalar_multiplications([(table, aligned_copy(big[o:o + 4096]), 4096) for o in (0, 4096, 8192)])
    for out, want in zip(outs, g["batched_3x4096"]):
        assert np.array_equal(out[0:4], limbs(want["x"])) and np.array_equal(out[4:8], limbs(want["y"]))
        assert np.array_equal(out[8:12], limbs(want["z"]))
    assert [mc.memory_stats(k)["srs_points_bytes"] for k in range(1, mc.N)] == before  # nothing below the split touched another context


def test_msm_skewed_2e20(mc, golden):
    """msm_r3.json's skewed scalar sets at 2^20 over a table registered EXPLICITLY: it stays whole on context 0, which serves its slice from it,
    while the other contexts register theirs on first sight"""
    import bench
    g = golden("msm_r3.json")
    n = 1 << 20
    h, table = mc.srs_generate(limbs(g["srs_secret_mont"]), n, want_host_table=True)  # registered explicitly: whole on context 0
    for kind in bench.SKEWED_KINDS:
        case = g["skewed_2e20"][kind]
        sc = aligned_copy(bench.skewed_scalars(kind, n))
        assert sha(sc) == case["scalars_sha256"], kind
        _check(mc.pippenger(sc, table, n), case)
    mc.srs_release(h)


def test_msm_segments_ragged_and_offset(mc, oracle, golden):
    """msm_r4.json: prefixes of a 2^21-point SRS (2^19 + 3 ragged, 2^20 + 8 and 2^21 across the table segments) and a slice that starts at
    point 5, on a table registered on first sight"""
    g = golden("msm_r4.json")
    N = 1 << 21
    h, table = mc.srs_generate(limbs(g["srs_secret_mont"]), N, want_host_table=True)
    mc.srs_release(h)
    assert sha(table[0::2]) == g["srs_digest_2097152"]
    scalars = oracle.random_scalars(SCALAR_SEED, N)
    t = aligned_copy(table)
    del table
    for case in g["prefixes"]:
        n = case["n"]
        _check(mc.pippenger(aligned_copy(scalars[:n]), t, n), case)
    sl = g["slice"]
    _check(mc.pippenger(aligned_copy(scalars[:sl["n"]]), t[2 * sl["offset"]:], sl["n"]), sl)
    n = g["prefixes"][0]["n"]
    outs = mc.batched_scalar_multiplications([(t, aligned_copy(scalars[:n]), n)] * 2)
    _check(outs[0], g["prefixes"][0])
    _check(outs[1], g["prefixes"][0])


def test_cross_slice_edge_cases(mc, tables, one_context):
    """partial sums that are equal (the fold doubles), opposite (the sum is the clean point at infinity), or a slice of zero scalars: the same
    bytes as one context"""
    _, _, _, rep, edge = tables
    t = aligned_copy(rep)
    for k, v in edge.items():
        got = mc.pippenger(v, t, EDGE_N)
        assert np.array_equal(got, one_context[k]), k
    assert one_context["opposite"][7] >> np.uint64(63) == 1 and not one_context["opposite"][:7].any()
    outs = mc.batched_scalar_multiplications([(t, v, EDGE_N) for v in edge.values()])
    for got, want in zip(outs, one_context["batch"]):
        assert np.array_equal(got, want)


def test_memory_is_split_and_cached(mc, tables):
    if mc.N != 2:
        pytest.skip("measured with two contexts")
    g, table, scalars, _, _ = tables
    n = 1 << 20
    mc.shutdown()
    mc.init_devices([0, 0])  # nothing cached: a freed copy of the table of an earlier test may lie at the same address
    t = aligned_copy(table)
    before = [mc.memory_stats(k) for k in range(2)]
    total_before = mc.memory_stats()
    _check(mc.pippenger(scalars, t, n), [c for c in g["cases"] if c["n"] == n][0])
    after = [mc.memory_stats(k) for k in range(2)]
    grew = [a["srs_points_bytes"] - b["srs_points_bytes"] for a, b in zip(after, before)]
    assert grew == [n // 2 * 64] * 2, grew  # each context holds its half of the points (one context: n * 64)
    assert sum(grew) == mc.memory_stats()["srs_points_bytes"] - total_before["srs_points_bytes"]
    for f in after[0]:
        assert mc.memory_stats()[f] == after[0][f] + after[1][f], f
    _check(mc.pippenger(scalars, t, n), [c for c in g["cases"] if c["n"] == n][0])
    assert [mc.memory_stats(k) for k in range(2)] == after  # the second call hit every context's cache


def test_everything_else_stays_on_context_0(mc, oracle, golden):
    """a resident PLONK proof (1024 gates) and the transforms of test_ntt_vs_oracle_all_kinds' sizes, with several contexts bound"""
    if mc.N != 2:
        pytest.skip("checked with two contexts")
    from barretenberg_amd.plonk import Prover, bench_circuit, proof_lines, to_montgomery_limbs
    before = mc.memory_stats(1)
    tr = golden("plonk_trace.json")
    secret = 0x0123456789ABCDEF0F1E2D3C4B5A6978FEDCBA98765432100123456789ABCDEF
    hs = mc.srs_generate(to_montgomery_limbs([secret % FR_MODULUS])[0], 65536)
    state = bench_circuit(1024, int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)).preprocess()
    P = Prover(mc, state, hs)
    try:
        assert proof_lines(state["n"], P.construct_proof()) == golden("plonk_proofs.json")["proofs"]["1024"][:26]
    finally:
        P.destroy()
    mc.srs_release(hs)
    import torch
    const = oracle.random_scalars(CONST_SEED, 1)[0]
    # the host-buffer entry (sizes up to the host threshold are answered on the host, as in any process) and the device entry (always the kernels);
    # the host thresholds are left as they are, so later modules still read them from the environment
    for log2n in (1, 2, 3, 4, 5, 8, 10, 11, 12, 13):
        co = noncanonical(oracle.random_scalars(NTT_SEED + log2n, 1 << log2n), FR_MODULUS)
        for kind in NTT_KINDS:
            want = oracle.ntt(co, kind, const)
            assert np.array_equal(mc.ntt(co.copy(), kind, const), want), (log2n, kind)
            d = torch.from_numpy(co.copy().view(np.int64)).cuda()
            mc.ntt_device(d.data_ptr(), 1 << log2n, kind, const)
            torch.cuda.synchronize()
            assert np.array_equal(d.cpu().numpy().view(np.uint64), want), (log2n, kind, "device")
    assert mc.memory_stats(1) == before  # context 1 was not touched


def test_split_batch_with_a_null_job(mc, tables):
    """the checks of a split batch behave as one context's: unequal sizes leave every output untouched; a null job ends the batch with the
    pipeline's text, and the outputs one context would have finished by then (job 0 of three, with job 2 null) are written"""
    import ctypes as C
    from barretenberg_amd.bbgpu import MsmJob, _ptr
    g, table, scalars, _, _ = tables
    n = 1 << 17
    t = aligned_copy(table[:2 * n])
    sc = [aligned_copy(scalars[k * n:(k + 1) * n]) for k in range(3)]
    want = [mc.pippenger(s, t, n) for s in sc[:2]]
    arr = (MsmJob * 3)()
    for j, s in zip(arr, sc):
        j.points, j.scalars, j.num_elements = _ptr(t), _ptr(s), n
    arr[2].num_elements = n - 8
    assert mc.lib.bbgpu_msm_g1_batch(arr, 3) == -3
    assert "each scalar mul must be same size" in mc.lib.bbgpu_last_error().decode()
    assert not any(any(j.output) for j in arr)
    arr[2].num_elements = n
    arr[2].scalars = C.cast(None, type(arr[2].scalars))
    assert mc.lib.bbgpu_msm_g1_batch(arr, 3) == -3
    assert mc.lib.bbgpu_last_error().decode() == "null scalars/points in job 2"
    assert np.array_equal(np.array(list(arr[0].output), dtype=np.uint64), want[0])
    assert not any(arr[1].output) and not any(arr[2].output)
    assert mc.fault_stats()["slots_pending"] == 0


def test_a_failing_context_is_reported_and_drained(mc, tables):
    """an injected failure (bbgpu_fault_inject: a HIP call fails in software, the device is not touched) in whichever context meets it first:
    BBGPU_ERR_HIP naming a context, nothing left in flight, and the next identical call returns the reference point"""
    if mc.N != 2:
        pytest.skip("checked with two contexts")
    from barretenberg_amd import BbGpuError
    g, table, scalars, _, _ = tables
    n = 1 << 20
    case = [c for c in g["cases"] if c["n"] == n][0]
    mc.shutdown()
    mc.init_devices([0, 0])  # a freshly bound pair: the next allocation is a table upload in one of the contexts
    t = aligned_copy(table)
    for spec in ("alloc:0", "h2d:0"):  # h2d: the tables are resident by then, the scalars' upload fails
        mc.fault_inject(spec)
        with pytest.raises(BbGpuError, match=r"bbgpu error -1: context [01] \(device 0\): "):
            mc.pippenger(scalars, t, n)
        st = mc.fault_stats()
        assert st["fired"] == 1 and st["armed"] == 0 and st["slots_pending"] == 0, (spec, st)
        _check(mc.pippenger(scalars, t, n), case)
    mc.fault_inject(None)


def test_shim_reference_calling_pattern_multi_context(tmp_path):
    """tests/cpp/test_shim_multi.cpp: the shim's batched_scalar_multiplications (three 2^17-point jobs) and pippenger from four OpenMP threads,
    with two contexts on device 0 -- the same points as with one"""
    pkg = os.path.join(ROOT, "barretenberg_amd")
    exe = str(tmp_path / "test_shim_multi")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-Wno-invalid-offsetof", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_shim_multi.cpp"),
                    "-L" + pkg, "-lbbshim", "-lbbgpu", "-Wl,-rpath," + pkg], check=True)
    outs = []
    for contexts in (1, 2):
        r = subprocess.run([exe, str(contexts)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, BBGPU_SHIM_STRICT="1", OMP_NUM_THREADS="4"))
        assert r.returncode == 0 and r.stdout.endswith("DONE\n"), (r.stdout[-500:], r.stderr[-1500:])
        lines = r.stdout.split("\n")
        assert lines[0] == "contexts %d" % contexts
        outs.append(lines[1:])
    assert len(outs[0]) == 2 * (3 + 4) + 2
    assert outs[0] == outs[1]


def test_two_real_devices(mc, tables):
    if mc.N != 2:
        pytest.skip("checked once")
    if mc.device_count() < 2:
        pytest.skip("one GPU on this machine: devices=[0, 1] not run")
    g, table, scalars, _, _ = tables
    n = 1 << 20
    mc.shutdown()
    try:
        mc.init_devices([0, 1])
        assert mc.num_contexts() == 2
        _check(mc.pippenger(scalars, aligned_copy(table), n), [c for c in g["cases"] if c["n"] == n][0])
    finally:
        mc.shutdown()
        mc.init_devices([0, 0])
