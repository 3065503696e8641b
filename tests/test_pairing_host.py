"""The host pairing (csrc/host_pairing.hpp through bbgpu_host_pairing / bbgpu_host_pairing_check) and the G2 half of the transcript reader: CPU tests,
no GPU.  The reference's own known answer is a data fixture (tests/golden/pairing_kats.json); multiples come from the oracle (G1) and from written
transcripts (x * G2, the only way a caller obtains G2 points from the library)."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FQ, FR, to_int
from tests.srs_check_cases import g2_of, secret_plus_one
from tests.util import limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


def mont(oracle, hexwords):
    raw = limbs(hexwords).reshape(-1, 4)
    return np.concatenate([oracle.to_mont(FQ, r) for r in raw])


def fq12_one(oracle):
    one = np.zeros((12, 4), dtype=np.uint64)
    one[0] = oracle.const(FQ, "one")
    return one


def neg_point(oracle, p):
    q = np.array(p[:8], dtype=np.uint64)
    q[4:8] = oracle.neg(FQ, q[4:8])
    return q


def g2_generator(oracle, path, num_g1):
    """the transcript's FIRST G2 record (the generator), parsed here from the format description: four coordinates of four 64-bit limbs, least
    significant limb first, every limb big-endian, not in Montgomery form"""
    raw = open(path, "rb").read()[28 + 64 * num_g1:28 + 64 * num_g1 + 128]
    words = np.array([int.from_bytes(raw[8 * i:8 * i + 8], "big") for i in range(16)], dtype=np.uint64).reshape(4, 4)
    return np.concatenate([oracle.to_mont(FQ, w) for w in words])


def test_pairing_reproduces_the_references_constants(lib, oracle):
    """reduced_ate_pairing_check_against_constants (and any further recorded pairs), byte for byte"""
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_kats.json")))["kats"]
    assert kats
    for kat in kats:
        got = lib.host_pairing(mont(oracle, kat["p"]), mont(oracle, kat["q"]))
        want = mont(oracle, kat["e"]).reshape(12, 4)
        assert got.tobytes() == want.tobytes(), kat["name"]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_bilinearity(lib, oracle, tmp_path, seed):
    a, b = oracle.random_scalars(seed, 2)
    ab = oracle.mul(FR, a, b)
    G = oracle.g1_one_affine()
    Q = g2_of(lib, oracle, tmp_path, oracle.const(FR, "one"), "one.dat")  # 1 * G2
    aP, abP = oracle.g1_scalar_mul(G, a)[:8], oracle.g1_scalar_mul(G, ab)[:8]
    bQ, abQ = g2_of(lib, oracle, tmp_path, b, "b.dat"), g2_of(lib, oracle, tmp_path, ab, "ab.dat")
    e1, e2, e3 = lib.host_pairing(aP, bQ), lib.host_pairing(abP, Q), lib.host_pairing(G, abQ)
    assert e1.tobytes() == e2.tobytes() == e3.tobytes()
    one = fq12_one(oracle)
    assert lib.host_pairing(G, Q).tobytes() != one.tobytes()
    inf = np.zeros(8, dtype=np.uint64)
    inf[7] = np.uint64(1 << 63)
    assert lib.host_pairing(inf, Q).tobytes() == one.tobytes()
    assert lib.host_pairing_check(np.stack([aP, neg_point(oracle, aP)]), np.stack([bQ, bQ]))
    assert not lib.host_pairing_check(np.stack([aP, aP]), np.stack([bQ, bQ]))
    assert lib.host_pairing_check(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 16), dtype=np.uint64))  # the empty product


def test_transcript_halves_pair_up(lib, oracle, tmp_path):
    """the reference's own test shape (read_transcript_loads_well_formed_srs): e(-x G, G2) e(G, x G2) = 1 on a written and re-read transcript, and
    not with the transcript of x + 1"""
    n = 64
    x = oracle.random_scalars(0x5EED, 1)[0]
    table = oracle.point_table(oracle.make_srs(x, n))
    path, path1 = str(tmp_path / "t.dat"), str(tmp_path / "t1.dat")
    lib.write_transcript(path, table, n, x)
    lib.write_transcript(path1, table, n, secret_plus_one(oracle, x))
    back = lib.read_transcript(path, n)
    assert np.array_equal(back, table)
    G2 = g2_generator(oracle, path, n - 1)
    ps = np.stack([neg_point(oracle, back[2]), back[0]])
    assert lib.host_pairing_check(ps, np.stack([G2, lib.transcript_read_g2(path)]))
    assert not lib.host_pairing_check(ps, np.stack([G2, lib.transcript_read_g2(path1)]))
    assert to_int(lib.transcript_read_g2(path)) != to_int(lib.transcript_read_g2(path1))


def test_pairing_argument_errors(lib, tmp_path):
    from barretenberg_amd import BbGpuError
    with pytest.raises(BbGpuError):
        lib.transcript_read_g2(str(tmp_path / "missing.dat"))
    short = tmp_path / "short.dat"
    short.write_bytes(b"\0" * 20)
    with pytest.raises(BbGpuError):
        lib.transcript_read_g2(str(short))


def test_pairing_code_under_sanitizers(oracle, tmp_path):
    """csrc/host_pairing.hpp and csrc/host_srs_check.hpp built into a stand-alone program with AddressSanitizer + UBSan (CPU build, its own main, no
    preloaded runtime): the known answer, the bilinearity cases and one host SRS check at n = 64 (tests/cpp/test_pairing_host.cpp)"""
    exe = str(tmp_path / "bbgpu_test_pairing_host")
    ob = os.path.join(ROOT, "oracle", "_build")
    base = ["g++", "-std=c++17", "-O1", "-g"]
    tail = ["-o", exe, os.path.join(ROOT, "tests", "cpp", "test_pairing_host.cpp"), "-L" + ob, "-loracle", "-Wl,-rpath," + ob, "-pthread"]
    b = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + tail, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        b = subprocess.run(base + tail, capture_output=True, text=True)  # an image without the sanitizer runtime still runs the program
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "pairing_kats.json")], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
