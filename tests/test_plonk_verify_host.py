"""bbgpu_host_plonk_verify_batch (csrc/host_plonk_verify.hpp): the batched PLONK verifier on the host -- the definition the GPU entry's reports are
compared with field for field (tests/test_gpu_plonk_verify.py).  CPU tests, no GPU.  Every expected verdict is the REFERENCE's
Verifier::verify_proof on the same bytes (tests/golden/plonk_verify.json, tools/gen_plonk_verify_golden.py), never this code's own."""
import os
import subprocess

import numpy as np
import pytest

from tests.plonk_verify_cases import BAD_POINT, NONE, ROOT, SEED, ZERO_EVAL, fields, fixture, mixed_batch, row, row_ids, whole


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


def verify(lib, circuit, proofs, seed=SEED, locate=True):
    g2_x, circuits, _ = fixture()
    c = circuits[circuit]
    return lib.host_plonk_verify_batch(c["n"], c["widgets"], c["vk"], g2_x, proofs, seed, locate)


@pytest.mark.parametrize("r", fixture()[2], ids=row_ids())
def test_every_fixture_row_gets_the_reference_verdict(lib, r):
    rep = verify(lib, r["circuit"], r["proof"])
    assert int(rep.status[0]) == r["status"], r["tamper"]
    assert rep.ok == bool(r["verdict"]), (r["tamper"], fields(rep))
    if r["status"]:
        assert fields(rep) == dict(count=1, bad_status=1, first_bad_status=0, pairing_checked=1, pairing_ok=1, first_bad_proof=NONE)
        assert int(rep.a[7]) >> 63 and int(rep.b[7]) >> 63  # nothing was summed
    else:
        assert fields(rep) == dict(count=1, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=r["verdict"],
                                   first_bad_proof=NONE if r["verdict"] else 0)


def test_the_representative_r_of_zero_is_judged_by_the_pairing(lib):
    """fr::eq compares words (field.hpp:166-170): sigma_1_eval = r is not ZERO_EVAL, the reference goes on and rejects at the pairing"""
    z, r = row("standard/32", "sigma_1_eval_zero"), row("standard/32", "sigma_1_eval_r")
    assert (z["status"], z["verdict"], r["status"], r["verdict"]) == (ZERO_EVAL, 0, 0, 0)
    assert int(verify(lib, "standard/32", z["proof"]).status[0]) == ZERO_EVAL
    rep = verify(lib, "standard/32", r["proof"])
    assert int(rep.status[0]) == 0 and rep.pairing_ok == 0


@pytest.mark.parametrize("count,bad", [
    (2, {0: "neg_Z_1"}), (2, {1: "plus_one_w_l_eval"}), (3, {1: "double_T_LO"}), (3, {0: "neg_PI_Z", 2: "neg_W_L"}),
    (17, {0: "plus_one_linear_eval"}), (17, {16: "neg_T_MID"}), (17, {8: "double_W_O"}), (17, {5: "infinity_W_L", 11: "neg_PI_Z_OMEGA"}),
    (17, {3: "off_curve_W_R", 9: "neg_Z_1", 12: "sigma_1_eval_zero"}), (17, {4: "off_curve_PI_Z"}), (17, {})])
def test_mixed_batches(lib, count, bad):
    proofs = mixed_batch(count, bad)
    rep = verify(lib, "standard/32", proofs)
    want_status = [row("standard/32", bad[j])["status"] if j in bad else 0 for j in range(count)]
    assert [int(v) for v in rep.status] == want_status
    flagged = [j for j in range(count) if want_status[j]]
    failing = [j for j in sorted(bad) if not want_status[j]]  # status 0, rejected by the reference: the pairing's to find
    assert fields(rep) == dict(count=count, bad_status=len(flagged), first_bad_status=flagged[0] if flagged else NONE, pairing_checked=1,
                               pairing_ok=0 if failing else 1, first_bad_proof=failing[0] if failing else NONE)
    assert rep.ok == (not bad)
    plain = verify(lib, "standard/32", proofs, locate=False)
    assert fields(plain) == dict(fields(rep), first_bad_proof=NONE) and whole(plain)["a"] == whole(rep)["a"] and whole(plain)["b"] == whole(rep)["b"]


def test_one_seed_one_report(lib):
    proofs = mixed_batch(3, {1: "neg_Z_1"})
    r1, r2 = verify(lib, "standard/32", proofs), verify(lib, "standard/32", proofs)
    assert whole(r1) == whole(r2) and [int(v) for v in r1.seed] == [int(v) for v in SEED]
    other = verify(lib, "standard/32", proofs, seed=SEED + np.uint64(1))
    assert fields(other) == fields(r1) and whole(other)["a"] != whole(r1)["a"] and whole(other)["b"] != whole(r1)["b"]
    drawn = verify(lib, "standard/32", mixed_batch(2, {}), seed=None)
    assert drawn.ok and any(int(v) for v in drawn.seed)


def test_argument_errors(lib):
    from barretenberg_amd.bbgpu import BbGpuError
    g2_x, circuits, _ = fixture()
    c = circuits["standard/32"]
    good = mixed_batch(1, {})

    def code(**kw):
        a = dict(n=c["n"], widgets=c["widgets"], vk=c["vk"], g2_x=g2_x, proofs=good, seed=SEED, locate=False)
        a.update(kw)
        with pytest.raises(BbGpuError) as e:
            lib.host_plonk_verify_batch(a["n"], a["widgets"], a["vk"], a["g2_x"], a["proofs"], a["seed"], a["locate"])
        return int(str(e.value).split()[2].rstrip(":"))
    ERR_ARG, ERR_SIZE = -3, -2
    assert code(n=33) == ERR_SIZE and code(n=0) == ERR_SIZE
    assert code(widgets=3) == ERR_ARG and code(widgets=8) == ERR_ARG and code(widgets=6) == ERR_ARG
    bad_vk = c["vk"].copy()
    bad_vk[4, 0] += np.uint64(1)
    assert code(vk=bad_vk) == ERR_ARG
    bad_g2 = g2_x.copy()
    bad_g2[0] += np.uint64(1)
    assert code(g2_x=bad_g2) == ERR_ARG
    inf_g2 = g2_x.copy()
    inf_g2[11] |= np.uint64(1 << 63)
    assert code(g2_x=inf_g2) == ERR_ARG
    assert code(proofs=np.zeros((0, 120), dtype=np.uint64)) == ERR_ARG
    assert code(proofs=np.zeros(((1 << 14) + 1, 120), dtype=np.uint64)) == ERR_SIZE
    # unknown flag bits, null pointers: through the raw entry
    import ctypes as C
    from barretenberg_amd.bbgpu import PlonkVerifyReport
    f = lib.lib.bbgpu_host_plonk_verify_batch
    f.argtypes = [C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    vk, st, rep = np.ascontiguousarray(c["vk"]), np.zeros(1, dtype=np.uint32), PlonkVerifyReport()
    args = [c["n"], c["widgets"], vk.ctypes.data, g2_x.ctypes.data, good.ctypes.data, 1, SEED.ctypes.data, 0, st.ctypes.data, C.addressof(rep)]
    assert f(*args) == 0
    assert f(*(args[:7] + [2] + args[8:])) == ERR_ARG
    for k in (2, 3, 4, 8, 9):
        assert f(*(args[:k] + [None] + args[k + 1:])) == ERR_ARG, k


def test_an_infinite_key_point_contributes_nothing(lib):
    """Q_C of the bench circuit is the point at infinity with whatever bits the reference's accumulators held (tests/golden/infinity_commitments.json)"""
    g2_x, circuits, _ = fixture()
    vk = circuits["standard/32"]["vk"]
    assert int(vk[7, 7]) >> 63
    assert verify(lib, "standard/32", row("standard/32", "none")["proof"]).ok
    assert verify(lib, "zerowire/32", row("zerowire/32", "none")["proof"]).ok  # W_R = W_O = infinity in an honest proof


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/cpp/test_plonk_verify_host.cpp: the host twin as a stand-alone program (own main), built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "test_plonk_verify_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_plonk_verify_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", src, "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "plonk_verify.json")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_gpu_entry_checks_its_arguments_first(lib):
    """handles are host objects; argument errors are refused before a device is bound"""
    from barretenberg_amd.bbgpu import BbGpuError
    g2_x, circuits, _ = fixture()
    c = circuits["standard/32"]
    with pytest.raises(BbGpuError, match=" -2:"):
        lib.plonk_verifier_create(c["n"] + 1, 0, c["vk"], g2_x)
    with pytest.raises(BbGpuError, match=" -3:"):
        lib.plonk_verifier_create(c["n"], 3, c["vk"], g2_x)
    h = lib.plonk_verifier_create(c["n"], c["widgets"], c["vk"], g2_x)
    try:
        with pytest.raises(BbGpuError, match=" -3:"):
            lib.plonk_verify_batch(h + 1000, mixed_batch(1, {}), SEED)
        with pytest.raises(BbGpuError, match=" -3:"):
            lib.plonk_verify_batch(h, np.zeros((0, 120), dtype=np.uint64), SEED)
        with pytest.raises(BbGpuError, match=" -2:"):
            lib.plonk_verify_batch(h, np.zeros(((1 << 14) + 1, 120), dtype=np.uint64), SEED)
    finally:
        lib.plonk_verifier_destroy(h)
    with pytest.raises(BbGpuError, match=" -3:"):
        lib.plonk_verifier_destroy(h)
    # the diagnostic getter: a null pointer is refused; five wall times, zeros before the first call of the process
    import ctypes as C
    lib.lib.bbgpu_plonk_verify_last_timing.argtypes = [C.c_void_p]
    assert lib.lib.bbgpu_plonk_verify_last_timing(None) == -3
    t = lib.plonk_verify_last_timing()
    assert sorted(t) == ["fold_ms", "host_tail_ms", "msm_ms", "terms_ms", "total_ms"] and all(v >= 0 for v in t.values())


def test_without_a_device_the_gpu_entry_fails(lib):
    """no host path behind the GPU entry: BBGPU_ERR_HIP, and the handle stays usable"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from barretenberg_amd.bbgpu import BbGpuError
    g2_x, circuits, _ = fixture()
    c = circuits["standard/32"]
    h = lib.plonk_verifier_create(c["n"], c["widgets"], c["vk"], g2_x)
    try:
        for _ in range(2):
            with pytest.raises(BbGpuError, match=" -1:"):  # BBGPU_ERR_HIP
                lib.plonk_verify_batch(h, mixed_batch(1, {}), SEED)
    finally:
        lib.plonk_verifier_destroy(h)
