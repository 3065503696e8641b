"""CPU tests of the drop-in boundary: library loads, exports every symbol include/bbgpu.h declares, fails loudly
without a GPU, and the host-side tail arithmetic (bbgpu_g1_sum, no GPU needed) matches the oracle."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu, build_library
    build_library()
    return BbGpu(init=False)


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bbgpu.h")).read()
    declared = set(re.findall(r"\b(bbgpu_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"bbgpu_msm_job"}
    from barretenberg_amd.bbgpu import C_ABI_SYMBOLS
    assert declared == set(C_ABI_SYMBOLS), declared ^ set(C_ABI_SYMBOLS)
    for name in declared:
        assert hasattr(lib.lib, name), name


def test_no_torch_types_in_abi():
    hdr = open(os.path.join(ROOT, "include", "bbgpu.h")).read()
    assert "torch" not in hdr and "at::" not in hdr and "std::" not in hdr


def test_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from barretenberg_amd import BbGpuError
    with pytest.raises(BbGpuError, match="no HIP device"):
        lib.fft(np.zeros((64, 4), dtype=np.uint64))
    with pytest.raises(BbGpuError, match="no HIP device"):
        lib.pippenger(np.zeros((64, 4), dtype=np.uint64), np.zeros((128, 8), dtype=np.uint64), 64)


def test_product_does_not_import_oracle():
    """the product path may not route through oracle/ (SURVEY scope rule 3)"""
    pkg = os.path.join(ROOT, "barretenberg_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".h", ".hpp", ".cpp", "Makefile")):
                text = open(os.path.join(dp, f)).read()
                assert "pyoracle" not in text and "bn254_oracle" not in text and "liboracle" not in text and "_ref/" not in text, f


def test_g1_sum_matches_oracle(lib, oracle):
    one = oracle.g1_one_affine()
    pts = [oracle.g1_scalar_mul(one, s) for s in oracle.random_scalars(2024, 6)]
    acc = np.zeros(12, dtype=np.uint64)
    acc[7] = np.uint64(1 << 63)
    for p in pts:
        acc = oracle.g1_add(acc, p)
    want = oracle.g1_normalize(acc)
    got = lib.g1_sum(np.stack(pts))
    assert np.array_equal(got, want)
    # Jacobian (non-normalised) inputs, infinity entries, P + (-P), P + P
    from oracle.pyoracle import FQ
    d = oracle.g1_dbl(pts[0])
    inf = np.zeros(12, dtype=np.uint64)
    inf[7] = np.uint64(1 << 63)
    neg = pts[1].copy()
    neg[4:8] = oracle.neg(FQ, pts[1][4:8])
    got = lib.g1_sum(np.stack([d, inf, pts[1], neg, pts[2], pts[2]]))
    want = oracle.g1_normalize(oracle.g1_add(d, oracle.g1_dbl(pts[2])))
    assert np.array_equal(got, want)
    assert int(lib.g1_sum(np.stack([pts[3], _neg(oracle, pts[3])]))[7]) >> 63 == 1
    assert int(lib.g1_sum(np.zeros((0, 12), dtype=np.uint64))[7]) >> 63 == 1


def _neg(oracle, p):
    from oracle.pyoracle import FQ
    q = p.copy()
    q[4:8] = oracle.neg(FQ, p[4:8])
    return q


def test_host_field_code_matches_oracle(tmp_path):
    """fe.hpp / g1.hpp (the code the kernels run) compiled for the host and checked against the oracle"""
    exe = str(tmp_path / "bbgpu_test_fe_host")
    src = os.path.join(ROOT, "tests", "cpp", "test_fe_host.cpp")
    ob = os.path.join(ROOT, "oracle", "_build")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, src, "-L" + ob, "-loracle", "-Wl,-rpath," + ob], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-2000:]


REFERENCE_SYMBOLS = [  # SURVEY 8b, taken from `nm` on the built reference objects
    "_ZN12barretenberg21scalar_multiplication9pippengerEPNS_5fieldINS_8FrParamsEE7field_tEPNS_5groupINS1_INS_13Bn254FqParamsEEES3_NS_13Bn254G1ParamsEE14affine_elementEmm",
    "_ZN12barretenberg21scalar_multiplication30batched_scalar_multiplicationsEPNS0_20multiplication_stateEm",
    "_ZN12barretenberg21polynomial_arithmetic3fftEPNS_5fieldINS_8FrParamsEE7field_tERKNS_17evaluation_domainE",
    "_ZN12barretenberg21polynomial_arithmetic4ifftEPNS_5fieldINS_8FrParamsEE7field_tERKNS_17evaluation_domainE",
    "_ZN12barretenberg21polynomial_arithmetic9coset_fftEPNS_5fieldINS_8FrParamsEE7field_tERKNS_17evaluation_domainE",
    "_ZN12barretenberg21polynomial_arithmetic10coset_ifftEPNS_5fieldINS_8FrParamsEE7field_tERKNS_17evaluation_domainE",
    "_ZN12barretenberg21polynomial_arithmetic17fft_with_constantEPNS_5fieldINS_8FrParamsEE7field_tERKNS_17evaluation_domainERKS4_",
    "_ZN12barretenberg21polynomial_arithmetic18ifft_with_constantEPNS_5fieldINS_8FrParamsEE7field_tERKNS_17evaluation_domainERKS4_",
    "_ZN12barretenberg21polynomial_arithmetic23coset_fft_with_constantEPNS_5fieldINS_8FrParamsEE7field_tERKNS_17evaluation_domainERKS4_",
]


def test_shim_defines_reference_symbols(lib):
    """the C++ shim exports exactly the mangled hot-path symbols of the reference (link-time drop-in)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "barretenberg_amd", "shim")], check=True, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "barretenberg_amd", "libbbshim.so")],
                         capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T"}
    assert set(REFERENCE_SYMBOLS) <= defined


def test_transcript_reader_matches_reference_format(tmp_path):
    """bbgpu_transcript_read_g1 (io.hpp:36-182 restated, host code) on a transcript written in the reference's format: the table equals
    generator + x^k G in Montgomery form with the endomorphism partners -- the array the reference's ReferenceString holds.
    The file comes from the reference's own code path when its test-only build is present (oracle/_ref/plonk_cpu transcript), and is
    always cross-checked against a writer restated here from the format description."""
    import subprocess
    from barretenberg_amd import BbGpu
    from oracle.pyoracle import FQ, Oracle, from_int
    O = Oracle()
    G = BbGpu(init=False)
    n = 64
    secret = 0x0123456789ABCDEF0F1E2D3C4B5A6978FEDCBA98765432100123456789ABCDEF
    x_mont = O.to_mont(1, from_int(secret))
    srs = O.make_srs(x_mont, n)  # x^i G, i < n, Montgomery
    want = O.point_table(srs)
    # writer restated from the format: manifest of seven big-endian u32, then x, y as 4 limbs (limb 0 first), each limb big-endian, plain form
    path = str(tmp_path / "t.dat")
    with open(path, "wb") as fh:
        for v in (0, 1, n - 1, 2, n - 1, 2, 0):
            fh.write(int(v).to_bytes(4, "big"))
        for i in range(1, n):
            for c in (srs[i][0:4], srs[i][4:8]):
                plain = O.from_mont(FQ, c)
                for limb in plain:
                    fh.write(int(limb).to_bytes(8, "big"))
        fh.write(bytes(256 + 64))
    got = G.read_transcript(path, n)
    assert np.array_equal(got, want)
    exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
    if os.path.exists(exe):
        ref_path = str(tmp_path / "ref.dat")
        subprocess.run([exe, "transcript", ref_path, str(n - 1)], check=True, stdout=subprocess.DEVNULL)
        assert np.array_equal(G.read_transcript(ref_path, n), want)
    with pytest.raises(Exception):
        G.read_transcript(path, n + 5)  # more points than the file holds


def test_shim_host_members_match_oracle(oracle, tmp_path):
    """the shim's host-only TU-mates (no caller on the prover path; the reference's benches and tests link them) on seeded inputs"""
    from oracle.pyoracle import FR
    subprocess.run(["make", "-C", os.path.join(ROOT, "barretenberg_amd", "shim")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    exe = str(tmp_path / "bbgpu_test_shim_host")
    pkg = os.path.join(ROOT, "barretenberg_amd")
    # the shim's own translation unit is compiled INTO the test with AddressSanitizer + UBSan (CPU build); plain link against libbbshim.so if the image has no sanitizer runtime
    san = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                          os.path.join(ROOT, "tests", "cpp", "test_shim_host.cpp"), os.path.join(pkg, "shim", "bb_shim.cpp"), "-L" + pkg, "-lbbgpu", "-Wl,-rpath," + pkg],
                         capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_shim_host.cpp"), "-L" + pkg, "-lbbshim", "-lbbgpu",
                        "-Wl,-rpath," + pkg], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0")).stdout
    assert "pipint ok" in out and "pippre ok" in out and "piplow ok" in out
    vec, width, raw = {}, {}, {}
    for line in out.splitlines():
        t = line.split()
        if t[0] == "width":
            width[int(t[1])] = int(t[2])
        elif t[0] in ("pipint", "pippre", "piplow"):
            assert t[1] == "ok", "pippenger_internal / alt_pippenger_internal / the plain-table entries differ from pippenger() or from (sum k_i i) G"
        elif t[0] in ("pre", "base", "prerounds"):
            raw.setdefault(t[0], []).append(t[1:])
        elif t[0].startswith(("wnaf", "skew", "state", "iter")):
            raw.setdefault(t[0], []).append(t[1:])
        else:
            vec.setdefault(t[0], []).append(np.array([int(x, 16) for x in t[2:6]], dtype=np.uint64))
    for n, w in width.items():
        assert w == oracle.optimal_bucket_width(n), n  # scalar_multiplication.cpp:21-81 via the oracle (2^20 -> 15, 2^16 -> 12, 1 -> 1)
    assert width[1 << 20] == 15 and width[1 << 16] == 12 and width[131072] == 15 and width[8192] == 10 and width[10000] == 10 and width[1] == 1
    a, b, g = np.stack(vec["a"]), np.stack(vec["b"]), vec["g"]
    n = a.shape[0]
    canon = lambda x: oracle.reduce_once(FR, oracle.reduce_once(FR, oracle.reduce_once(FR, x)))  # inputs < 2^254 < 4r
    for i in range(n):
        assert np.array_equal(vec["add"][i], oracle.add(FR, canon(a[i]), canon(b[i])))
        assert np.array_equal(vec["mul"][i], canon(oracle.mul(FR, a[i], b[i])))
    work = canon(g[0])
    for i in range(n):  # polynomial_arithmetic.cpp:81-102
        assert np.array_equal(vec["scale"][i], canon(oracle.mul(FR, a[i], work))), i
        work = canon(oracle.mul(FR, work, g[1]))
    acc = oracle.const(FR, "generator")
    for _ in range(6):
        acc = oracle.sqr(FR, acc)
    root = oracle.root_of_unity(3)
    for i in range(8):  # :104-127
        assert np.array_equal(vec["subgroup"][i], canon(acc)), i
        acc = oracle.mul(FR, acc, root)
    assert np.array_equal(np.stack(vec["fft_serial"]), oracle.ntt(a, "fft"))  # :37-79 computes the same transform as fft()
    # compute_wnaf_state / compute_next_bucket_index (scalar_multiplication.cpp:83-88, 265-308) against the oracle's split and digit functions
    # (pinned by the reference's own vectors, tests/golden/endo_wnaf.json)
    k = np.stack(vec["k"])
    m = k.shape[0]
    for forced in (0, 7):
        bits = forced or oracle.optimal_bucket_width(m)
        rounds = (127 + bits) // (bits + 1)
        assert [int(x) for x in raw["wnafstate"][[0, 7].index(forced)]] == [forced, 2 * m, rounds, 1 << bits, bits + 1]
        table = np.array([[int(x, 16) for x in row[1:]] for row in raw["wnaf%d" % forced]], dtype=np.uint32)
        skew = [int(x) for x in raw["skew%d" % forced][0][1:]]
        endo = np.stack(vec["endo%d" % forced])
        assert table.shape == (rounds, 2 * m)
        for i in range(m):
            k1, k2 = oracle.split_endo(k[i])
            assert np.array_equal(endo[i][:2], k1) and np.array_equal(endo[i][2:], k2), i
            for half, kk in enumerate((k1, k2)):
                want, want_skew = oracle.fixed_wnaf(kk, bits + 1)
                assert np.array_equal(table[:, 2 * i + half], want), (forced, i, half)
                assert skew[2 * i + half] == want_skew
        first = int(table[0, 0])
        assert [int(x) for x in raw["state%d" % forced][0]] == [0, 1, 1, first >> 31, first & 0x0fffffff]
        e5 = int(table[0, 5])  # (the precomputed-table check follows the loop)
        assert raw["iter%d" % forced][0][1:3] == [str(e5 >> 31), str(e5 & 0x0fffffff)] and int(raw["iter%d" % forced][0][3], 16) == e5
    # generate_pippenger_precompute_table (:90-129): round i of the table holds 2^(4 (i + 1)) P_j (c = 3 -> 4 doublings per round, 32 rounds), most significant table first
    from oracle.pyoracle import FQ
    assert raw["prerounds"][0] == ["0", "32", "1", "1"]
    base = {int(r[1]): np.array([int(x, 16) for x in r[2:10]], dtype=np.uint64) for r in raw["base"]}
    one = oracle.const(FQ, "one")
    for r in raw["pre"]:
        i, j = int(r[0]), int(r[1])
        p = np.concatenate([base[j], one])
        for _ in range(4 * (i + 1)):
            p = oracle.g1_dbl(p)
        assert np.array_equal(oracle.g1_normalize(p)[:8], np.array([int(x, 16) for x in r[2:10]], dtype=np.uint64)), (i, j)


def test_shim_covers_the_replaced_translation_units(golden):
    """INTEGRATION recipe A replaces two whole translation units: every extern of polynomial_arithmetic.o is defined by the shim, and
    and every extern of scalar_multiplication.o (the CPU algorithm's own machinery and the precomputed family as host code).  The externs are those of
    tests/golden/reference_build.json (tools/gen_ref_build_golden.py), which must equal the reference objects compiled in place (oracle/_ref/obj) where they are built."""
    want = {k: set(v) for k, v in golden("reference_build.json")["externs"].items()}
    obj = os.path.join(ROOT, "oracle", "_ref", "obj")
    pa, sm = os.path.join(obj, "polynomials", "polynomial_arithmetic.o"), os.path.join(obj, "curves", "bn254", "scalar_multiplication.o")

    def externs(path, dynamic=False):
        out = subprocess.run(["nm"] + (["-D"] if dynamic else []) + ["--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and "barretenberg" in l.split()[2]}

    if os.path.exists(pa) and os.path.exists(sm):
        assert externs(pa) == want["polynomial_arithmetic"] and externs(sm) == want["scalar_multiplication"], "stale fixture: rerun tools/gen_ref_build_golden.py"
    shim = externs(os.path.join(ROOT, "barretenberg_amd", "libbbshim.so"), dynamic=True)
    assert want["polynomial_arithmetic"] <= shim, sorted(want["polynomial_arithmetic"] - shim)
    assert want["scalar_multiplication"] <= shim, sorted(want["scalar_multiplication"] - shim)  # since round 2 incl. the CPU algorithm's own machinery and the precomputed family


def test_transcript_writer_matches_the_reference_writer(lib, oracle, golden, tmp_path):
    """bbgpu_transcript_write (io.hpp:36-182 restated for writing, G2 half computed by csrc/host_g2.hpp) against the file the
    REFERENCE's own code wrote for the same secret (oracle/_ref/transcript.dat <- g1/g2::group_exponentiation in plonk_cpu): the G1
    bytes of the shared prefix and both G2 points -- x * G2 is the verifier's pairing input -- must be identical; and our reader
    reads our file back.  The reference file's bytes are those of tests/golden/reference_build.json (tools/gen_ref_build_golden.py), which must
    describe oracle/_ref/transcript.dat where that is built."""
    import hashlib
    from oracle.pyoracle import FR
    ref = golden("reference_build.json")["transcript"]
    ref_file = os.path.join(ROOT, "oracle", "_ref", "transcript.dat")
    if os.path.exists(ref_file):
        data = open(ref_file, "rb").read()
        num = int.from_bytes(data[16:20], "big")
        assert (data[0:28].hex(), hashlib.sha256(data[28:28 + 64 * ref["g1_prefix_points"]]).hexdigest(), data[28 + 64 * num:][:256].hex()) == \
            (ref["manifest_hex"], ref["g1_prefix_sha256"], ref["g2_hex"]), "stale fixture: rerun tools/gen_ref_build_golden.py"
    secret_raw = np.array([0x0123456789abcdef, 0xfedcba9876543210, 0x0f1e2d3c4b5a6978, 0x0123456789abcdef], dtype=np.uint64)  # oracle/plonk_driver.cpp secret()
    x = oracle.to_mont(FR, secret_raw)
    degree = 1025
    table = oracle.point_table(oracle.make_srs(x, degree))
    path = str(tmp_path / "transcript.dat")
    lib.write_transcript(path, table, degree, x)
    ours, manifest = open(path, "rb").read(), bytes.fromhex(ref["manifest_hex"])
    assert len(ours) == 28 + 64 * (degree - 1) + 256 + 64 and ref["g1_prefix_points"] == degree - 1
    assert int.from_bytes(ours[16:20], "big") == degree - 1 and int.from_bytes(ours[8:12], "big") == degree - 1
    assert ours[0:8] == manifest[0:8] and ours[12:16] == manifest[12:16] and ours[20:28] == manifest[20:28]  # numbers / G2 counts / start_from
    assert hashlib.sha256(ours[28:28 + 64 * (degree - 1)]).hexdigest() == ref["g1_prefix_sha256"]            # x G .. x^1024 G
    assert ours[28 + 64 * (degree - 1):][:256].hex() == ref["g2_hex"]                                        # G2, x G2
    assert np.array_equal(lib.read_transcript(path, degree), table)


def test_bench_input_generator_is_splitmix64():
    """bench.py's synthetic inputs are splitmix64 from state 0x9e3779b97f4a7c15, 4 outputs per scalar, limb 3 masked to 60 bits"""
    import bench
    M = (1 << 64) - 1

    def ref(state, count):
        out = []
        for _ in range(count):
            state = (state + 0x9E3779B97F4A7C15) & M
            z = state
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
            out.append(z ^ (z >> 31))
        return out
    got = bench.splitmix64(bench.SPLITMIX_GAMMA, 64)
    assert [int(v) for v in got] == ref(0x9E3779B97F4A7C15, 64)
    sc = bench.raw_scalars(16, bench.SPLITMIX_GAMMA)
    want = ref(0x9E3779B97F4A7C15, 64)
    for i in range(16):
        assert [int(v) for v in sc[i]] == want[4 * i:4 * i + 3] + [want[4 * i + 3] & 0x0FFFFFFFFFFFFFFF]
    assert all(sum(int(v) << (64 * k) for k, v in enumerate(s)) < (1 << 252) for s in sc)
    assert [int(v) for v in bench.limbs_of(pow(2, 512, bench.FR_MODULUS))] == [0x1BB8E645AE216DA7, 0x53FE3AB1E35C59E3, 0x8C49833D53BB8085, 0x0216D0B17F4E44A5]  # fr.hpp:49-52 r_squared


def test_bench_dump_outputs_are_exact_and_bounded(tmp_path):
    """bench.py --dump-outputs: uint64 limbs survive the float64 encoding exactly, the NTT sample is the same fixed set of distinct elements every
    time, and the files of a 2^20 run stay under the 64 MB limit"""
    import bench
    a = np.array([0, 1, 0xFFFFFFFF, 1 << 32, 0xFFFFFFFFFFFFFFFF, 0x30644E72E131A029], dtype=np.uint64)
    f = bench.u64_as_f64(a)
    assert f.dtype == np.float64 and f.shape == (6, 2)
    assert [int(lo) | (int(hi) << 32) for lo, hi in f] == [int(v) for v in a]
    n = 1 << 20
    idx = bench.ntt_dump_index(n)
    assert np.array_equal(idx, bench.ntt_dump_index(n)) and idx.shape == (bench.NTT_DUMP_SAMPLE,)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(bench.ntt_dump_index(64), np.arange(64))
    limbs = bench.raw_scalars(n, 0xF00D)[idx]
    arrays = {"msm_result": bench.u64_as_f64(np.arange(12, dtype=np.uint64)), "ntt_sample_index": idx.astype(np.float64),
              "ntt_fft": bench.u64_as_f64(limbs), "ntt_coset_fft": bench.u64_as_f64(limbs)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sum(os.path.getsize(tmp_path / "out" / (k + ".npy")) for k in arrays) <= bench.DUMP_LIMIT_BYTES
    for k, v in arrays.items():
        assert np.array_equal(np.load(tmp_path / "out" / (k + ".npy")), v)


# the only environment variables the library and the shim read: the deployment settings of INTEGRATION.md's first table and the testing
# hooks the suite sets.  Nothing else may select a kernel or a launch sequence.
ENV_ALLOWLIST = {
    "BBGPU_HOST_MSM_MAX", "BBGPU_HOST_NTT_MAX", "BBGPU_SRS_CACHE_BYTES", "BBGPU_TABLE_C", "BBGPU_STAGE_MAX_BYTES", "BBGPU_STAGE_THREADS",
    "BBGPU_HOST_MSM_SPLIT", "BBGPU_TRACE_SRS", "BBGPU_TABLE_MAX_BYTES", "BBGPU_FALLBACK_THREADS", "BBGPU_SRS_VALIDATE",
    "BBGPU_SHIM_STRICT", "BBGPU_SHIM_PROFILE", "BBGPU_SHIM_TRACE",
    "BBGPU_FAIL_AT", "BBGPU_TABLE_SEG_POINTS", "BBGPU_NTT_TABLE_BYTES", "BBGPU_STAGE_CHUNK_BYTES",
}
# the only BBGPU_* macros a preprocessor conditional of csrc may test: the portable field products (-DBBGPU_NO_MONT_ASM), the switch fe.hpp
# derives from it, and the helper start-up delay tests/cpp/test_host_sanitize.cpp builds with
BUILD_MACRO_ALLOWLIST = {"BBGPU_NO_MONT_ASM", "BBGPU_MONT_ASM", "BBGPU_COPY_POOL_TEST_DELAY"}


def test_library_reads_only_allowlisted_settings():
    """no environment variable or build macro selects a kernel, a launch sequence or a result: every getenv() of the library and the
    shim names an allowlisted deployment setting or testing hook, no #if in csrc tests another BBGPU_* macro, and the transform's
    phase ablation is gone"""
    src = os.path.join(ROOT, "barretenberg_amd", "csrc")
    shim = os.path.join(ROOT, "barretenberg_amd", "shim")
    files = [os.path.join(d, f) for d in (src, shim) for f in sorted(os.listdir(d)) if f.endswith((".hip", ".hpp", ".h", ".cpp"))]
    seen = set()
    for path in files:
        text = open(path, errors="replace").read()
        calls = re.findall(r"\bgetenv\s*\(", text)
        names = re.findall(r'\bgetenv\s*\(\s*"([A-Za-z0-9_]+)"\s*\)', text)
        assert len(names) == len(calls), (path, "getenv() without a literal name")
        for name in names:
            assert name in ENV_ALLOWLIST, (os.path.basename(path), name)
        seen.update(names)
        if path.startswith(src):
            for line in text.splitlines():
                m = re.match(r"\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)", line)
                if m:
                    for macro in re.findall(r"\bBBGPU_[A-Za-z0-9_]+", m.group(1).split("//")[0]):
                        assert macro in BUILD_MACRO_ALLOWLIST, (os.path.basename(path), line.strip())
    assert seen == ENV_ALLOWLIST, ENV_ALLOWLIST ^ seen  # the allowlist names nothing that is no longer read
    ntt = open(os.path.join(src, "ntt.hip")).read()
    assert "NTT_DEBUG_SKIP" not in ntt and "debug_skip" not in ntt.lower()


def test_environment_variable_table_is_generated_from_the_sources():
    """INTEGRATION.md lists every BBGPU_* variable the product reads; tools/gen_env_table.py --check fails when the list is stale"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_env_table.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr or r.stdout


def test_fault_injection_and_validation_entries_without_a_device():
    """the testing hooks of include/bbgpu.h are plain host code: a spec is parsed and armed without a device, a bad one is an argument error, the counters start
    at zero and nothing is alive; bbgpu_srs_set_validate(-1, x) sets the process default, an unknown handle is an argument error"""
    from barretenberg_amd import BbGpu, BbGpuError
    lib = BbGpu(init=False)
    for spec in ("alloc:0", "h2d:17", "d2h:3", "launch:123456789012"):
        lib.fault_inject(spec)
        st = lib.fault_stats()
        assert st["armed"] == 1 and st["fired"] == 0 and st["alloc_calls"] == st["h2d_calls"] == st["d2h_calls"] == st["launch_checks"] == 0
    for bad in ("alloc", "alloc:", "alloc:x", "free:1", "launch:1:2", ":3"):
        with pytest.raises(BbGpuError, match="not understood"):
            lib.fault_inject(bad)
    lib.fault_inject(None)
    st = lib.fault_stats()
    assert st["armed"] == 0 and st["live_allocations"] == 0 and st["live_bytes"] == 0 and st["slots_pending"] == 0
    lib.srs_set_validate(-1, True)
    lib.srs_set_validate(-1, False)
    with pytest.raises(BbGpuError):
        lib.srs_set_validate(5, True)
