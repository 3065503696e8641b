"""bbgpu_host_plonk_verify_multi (csrc/host_plonk_verify.hpp, verify_host_multi): proofs of several circuits under one x G2 in one batch, one pairing
check for all -- the definition bbgpu_plonk_verify_multi's reports are compared with field for field (tests/test_gpu_plonk_verify_multi.py).  CPU
tests, no GPU.  Expected verdicts are the REFERENCE's on the same bytes (tests/golden/plonk_verify.json), never this code's own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.plonk_verify_cases import NONE, ROOT, SEED, fields, fixture, mixed_batch, row, row_ids, whole
from tests.plonk_verify_multi_cases import CIRCUITS, honest, honest_batch, index, keys, other_g2, others_plus

ERR_ARG, ERR_SIZE = -3, -2


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


def verify(lib, labels, proofs, names=CIRCUITS, seed=SEED, locate=True):
    return lib.host_plonk_verify_multi(keys(names), fixture()[0], labels, proofs, seed, locate)


@pytest.mark.parametrize("r", fixture()[2], ids=row_ids())
def test_every_fixture_row_among_the_other_circuits_gets_the_reference_verdict(lib, r):
    """the honest proofs of the five other circuits plus the row under its own label, the row first, in the middle and last: the batch is good iff the
    reference accepted the row"""
    for where in ("first", "middle", "last"):
        labels, proofs, p = others_plus(r, where)
        rep = verify(lib, labels, proofs)
        assert [int(v) for v in rep.status] == [r["status"] if j == p else 0 for j in range(6)], (where, r["tamper"])
        assert rep.ok == bool(r["verdict"]), (where, r["tamper"], fields(rep))
        if r["status"]:
            assert fields(rep) == dict(count=6, bad_status=1, first_bad_status=p, pairing_checked=1, pairing_ok=1, first_bad_proof=NONE), where
        else:
            assert fields(rep) == dict(count=6, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=r["verdict"],
                                       first_bad_proof=NONE if r["verdict"] else p), where


def test_a_wrong_label_is_a_bad_proof(lib):
    """standard/32 / proof_of_extended_32 is the extended circuit's proof under the standard key: status 0, rejected by the reference.  The same bytes
    labelled extended/32 pass; labelled standard/32 they fail and are located"""
    r = row("standard/32", "proof_of_extended_32")
    assert (r["status"], r["verdict"]) == (0, 0)
    labels, proofs, p = others_plus(dict(r, circuit="extended/32"), "middle")
    rep = verify(lib, labels, proofs)
    assert rep.ok and not rep.status.any()
    labels = labels.copy()
    labels[p] = index("standard/32")
    rep = verify(lib, labels, proofs)
    assert fields(rep) == dict(count=6, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=0, first_bad_proof=p)


def test_exchanged_labels_of_two_circuits_of_the_same_n(lib):
    """standard/32 and mimc/30 are both of n = 32: honest proofs, each under the other's label"""
    proofs = np.stack([honest("standard/32"), honest("mimc/30")])
    right = np.array([index("standard/32"), index("mimc/30")], dtype=np.uint32)
    assert verify(lib, right, proofs).ok
    rep = verify(lib, right[::-1].copy(), proofs)
    assert fields(rep) == dict(count=2, bad_status=0, first_bad_status=NONE, pairing_checked=1, pairing_ok=0, first_bad_proof=0)


@pytest.mark.parametrize("bad", [{}, {1: "neg_Z_1", 5: "off_curve_W_R", 6: "plus_one_linear_eval"}], ids=["honest", "tampered"])
def test_one_circuit_equals_the_single_circuit_entry(lib, bad):
    """G = 1: the definition IS bbgpu_host_plonk_verify_batch's, the report equal in every field, a and b included"""
    g2_x, circuits, _ = fixture()
    c = circuits["standard/32"]
    proofs = mixed_batch(9, bad)
    for locate in (False, True):
        one = lib.host_plonk_verify_batch(c["n"], c["widgets"], c["vk"], g2_x, proofs, SEED, locate)
        multi = verify(lib, np.zeros(9, dtype=np.uint32), proofs, names=("standard/32",), locate=locate)
        assert whole(multi) == whole(one)
        assert multi.ok == (not bad)


def test_duplicate_keys(lib):
    """keys = [k, k], circuit[j] = j % 2 over 16 proofs of one circuit: the segmented sums against the plain one -- a, b and the verdict are the
    single-circuit report's"""
    g2_x, circuits, _ = fixture()
    c = circuits["standard/32"]
    proofs = honest_batch(np.full(16, index("standard/32")))
    labels = (np.arange(16) % 2).astype(np.uint32)
    for tamper in (None, "double_T_MID"):
        if tamper:
            proofs[10] = row("standard/32", tamper)["proof"]
        one = lib.host_plonk_verify_batch(c["n"], c["widgets"], c["vk"], g2_x, proofs, SEED, True)
        two = verify(lib, labels, proofs, names=("standard/32", "standard/32"))
        assert whole(two) == whole(one)
        assert two.ok == (tamper is None) and int(two.first_bad_proof) == (NONE if tamper is None else 10)


def test_argument_errors(lib):
    from barretenberg_amd.bbgpu import BbGpuError, PlonkVerifyKey, PlonkVerifyReport
    g2_x = fixture()[0]
    labels, proofs, _ = others_plus(row("standard/32", "none"), "first")

    def code(names=CIRCUITS, labels=labels, proofs=proofs, g2=g2_x, key_of=None):
        ks = keys(names)
        if key_of:
            ks = [key_of(k) for k in ks]
        with pytest.raises(BbGpuError) as e:
            lib.host_plonk_verify_multi(ks, g2, labels, proofs, SEED, False)
        words = str(e.value).split()
        assert len(words) > 3  # a text after "bbgpu error <code>:"
        return int(words[2].rstrip(":")), str(e.value)
    assert code(names=())[0] == ERR_ARG
    assert code(names=CIRCUITS * 11)[0] == ERR_SIZE  # 66 keys
    # 64 keys are legal; the last of them is mimc/30
    assert verify(lib, np.full(2, 63, dtype=np.uint32), np.tile(honest("mimc/30"), (2, 1)), names=CIRCUITS * 10 + CIRCUITS[:4]).ok
    bad_labels = labels.copy()
    bad_labels[4] = 6
    rc, text = code(labels=bad_labels)
    assert rc == ERR_ARG and "circuit[4]" in text
    assert code(labels=labels[:0], proofs=proofs[:0])[0] == ERR_ARG
    big = (1 << 14) + 1
    assert code(labels=np.zeros(big, dtype=np.uint32), proofs=np.zeros((big, 120), dtype=np.uint64))[0] == ERR_SIZE
    assert code(key_of=lambda k: (k[0] + 1, k[1], k[2]))[0] == ERR_SIZE
    assert code(key_of=lambda k: (k[0], 3, k[2]))[0] == ERR_ARG
    bad_g2 = g2_x.copy()
    bad_g2[0] += np.uint64(1)
    assert code(g2=bad_g2)[0] == ERR_ARG
    # unknown flag bits, null pointers: through the raw entry
    f = lib.lib.bbgpu_host_plonk_verify_multi
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    vks = [np.ascontiguousarray(vk) for _, _, vk in keys()]
    ks = (PlonkVerifyKey * 6)(*[PlonkVerifyKey(n, w, v.ctypes.data) for (n, w, _), v in zip(keys(), vks)])
    st, rep = np.zeros(6, dtype=np.uint32), PlonkVerifyReport()
    args = [C.addressof(ks), 6, g2_x.ctypes.data, labels.ctypes.data, proofs.ctypes.data, 6, SEED.ctypes.data, 0, st.ctypes.data, C.addressof(rep)]
    assert f(*args) == 0 and rep.pairing_ok == 1
    assert f(*(args[:7] + [2] + args[8:])) == ERR_ARG and lib.lib.bbgpu_last_error()
    for k in (0, 2, 3, 4, 8, 9):
        assert f(*(args[:k] + [None] + args[k + 1:])) == ERR_ARG and lib.lib.bbgpu_last_error(), k
    ks[2].vk = None
    assert f(*args) == ERR_ARG and lib.lib.bbgpu_last_error()


def test_standalone_program_under_sanitizers(tmp_path):
    """tests/cpp/test_plonk_verify_multi_host.cpp: verify_host_multi as a stand-alone program (own main), built with -fsanitize=address,undefined"""
    exe = str(tmp_path / "test_plonk_verify_multi_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_plonk_verify_multi_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", src, "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "plonk_verify.json")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_the_gpu_entry_checks_its_arguments_first(lib):
    """handles are host objects; every argument error of bbgpu_plonk_verify_multi is refused before a device is bound (this process never binds one)"""
    from barretenberg_amd.bbgpu import BbGpuError, PlonkVerifyReport
    g2_x, circuits, _ = fixture()
    hs = [lib.plonk_verifier_create(c["n"], c["widgets"], c["vk"], g2_x) for c in circuits.values()]
    labels, proofs, _ = others_plus(row("standard/32", "none"), "first")

    def code(handles=hs, labels=labels, proofs=proofs):
        with pytest.raises(BbGpuError) as e:
            lib.plonk_verify_multi(handles, labels, proofs, SEED)
        words = str(e.value).split()
        assert len(words) > 3
        return int(words[2].rstrip(":")), str(e.value)
    try:
        assert code(handles=[])[0] == ERR_ARG
        assert code(handles=hs * 11)[0] == ERR_SIZE
        assert code(handles=hs[:5] + [hs[5] + 1000])[0] == ERR_ARG
        assert code(handles=hs[:5] + [-1])[0] == ERR_ARG
        bad_labels = labels.copy()
        bad_labels[3] = 6
        rc, text = code(labels=bad_labels)
        assert rc == ERR_ARG and "circuit[3]" in text
        assert code(labels=labels[:0], proofs=proofs[:0])[0] == ERR_ARG
        big = (1 << 14) + 1
        assert code(labels=np.zeros(big, dtype=np.uint32), proofs=np.zeros((big, 120), dtype=np.uint64))[0] == ERR_SIZE
        # a handle under another reference string
        c = circuits["standard/32"]
        foreign = lib.plonk_verifier_create(c["n"], c["widgets"], c["vk"], other_g2())
        try:
            rc, text = code(handles=hs[:5] + [foreign])
            assert rc == ERR_ARG and "g2_x" in text
        finally:
            lib.plonk_verifier_destroy(foreign)
        # unknown flag bits, null pointers: through the raw entry
        f = lib.lib.bbgpu_plonk_verify_multi
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        hv = (C.c_int * 6)(*hs)
        st, rep = np.zeros(6, dtype=np.uint32), PlonkVerifyReport()
        args = [C.addressof(hv), 6, labels.ctypes.data, proofs.ctypes.data, 6, SEED.ctypes.data, 0, st.ctypes.data, C.addressof(rep)]
        assert f(*(args[:6] + [2] + args[7:])) == ERR_ARG and lib.lib.bbgpu_last_error()
        for k in (0, 2, 3, 7, 8):
            assert f(*(args[:k] + [None] + args[k + 1:])) == ERR_ARG and lib.lib.bbgpu_last_error(), k
    finally:
        for h in hs:
            lib.plonk_verifier_destroy(h)
    with pytest.raises(BbGpuError, match=" -3:"):
        lib.plonk_verify_multi(hs, labels, proofs, SEED)  # destroyed handles
