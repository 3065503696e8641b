"""GPU parity tests (-m gpu) of the resident polynomial helpers (poly.hip) and of the resident PLONK
prover (plonk.hip, SURVEY 8f #2 / BASELINE config 5), through the C ABI.  Bit-exact bar.

Checkers: oracle.pyoracle.PolyOracle (big-integer restatement, pinned by tests/golden/poly_ops.json = outputs of the
reference itself), the fixtures directly, size-independent properties at full size, and for the prover the reference's own
golden proofs (tests/golden/plonk_proofs.json) plus, when the reference build travelled to the box, its Verifier."""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FR_MODULUS, PolyOracle as P, to_int
from tests.util import noncanonical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gpu():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.shutdown()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()  # the helpers are asynchronous on the library's own (non-blocking) stream
    return t.cpu().numpy().view(np.uint64)


def hx(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return ["%064x" % to_int(r) for r in a]


# ------------------------------------------------------------------ helpers vs the reference's fixtures ---------------
def test_poly_helpers_match_reference_fixtures(gpu, torch, oracle, golden):
    for case in golden("poly_ops.json")["cases"]:
        n, seed = case["n"], case["seed"]
        v, z, w = oracle.random_scalars(seed, n), oracle.random_scalars(seed + 1, 1)[0], oracle.random_scalars(seed + 2, n)
        dv, dw = dev(torch, v), dev(torch, w)
        assert hx(gpu.evaluate_device(dv.data_ptr(), n, z))[0] == case["evaluate"]
        d = dv.clone()
        gpu.batch_invert_device(d.data_ptr(), n)
        assert hx(host(d)) == case["batch_invert"]
        dest = torch.zeros_like(dv)
        f = gpu.compute_kate_opening_coefficients_device(dv.data_ptr(), dest.data_ptr(), n, z)
        assert hx(host(dest)) == case["kate_dest"] and hx(f)[0] == case["kate_f"]
        out = torch.zeros_like(dv)
        gpu.mul_device(out.data_ptr(), dv.data_ptr(), dw.data_ptr(), n)
        assert hx(host(out)) == case["pointwise_mul"]
        l1 = torch.zeros((2 * n, 4), dtype=torch.int64, device="cuda")
        gpu.compute_lagrange_polynomial_fft_device(l1.data_ptr(), n, 2 * n)
        assert hx(host(l1)) == case["lagrange_l1_fft_2n"]
        for k, off, key in ((2, 3, "divide_vanishing_2n"), (4, 4, "divide_vanishing_4n")):
            c = dev(torch, oracle.random_scalars(seed + off, k * n))
            gpu.divide_by_pseudo_vanishing_polynomial_device(c.data_ptr(), n, k * n)
            assert hx(host(c)) == case[key]


# ------------------------------------------------------------------ helpers vs the big-integer oracle, ragged sizes -----
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 5000])
def test_scans_and_evaluate_vs_oracle(gpu, torch, oracle, n):
    """sizes around the run (8), workgroup (2048) and two-workgroup boundaries; inputs partly non-canonical ([r, 2r))"""
    v = noncanonical(oracle.random_scalars(0x5CA9 + n, n), FR_MODULUS)
    z = oracle.random_scalars(0x5CAA + n, 1)[0]
    dv = dev(torch, v)
    assert np.array_equal(gpu.evaluate_device(dv.data_ptr(), n, z), P.evaluate(v, z))
    out = torch.zeros_like(dv)
    for reverse in (False, True):
        for inclusive in (False, True):
            gpu.product_scan_device(dv.data_ptr(), out.data_ptr(), n, reverse, inclusive)
            assert np.array_equal(host(out), P.product_scan(v, reverse, inclusive)), (n, reverse, inclusive)
    f = gpu.compute_kate_opening_coefficients_device(dv.data_ptr(), out.data_ptr(), n, z)
    want, wf = P.kate_opening(v, z)
    assert np.array_equal(host(out), want) and np.array_equal(f, wf)
    # in place
    d2 = dv.clone()
    gpu.compute_kate_opening_coefficients_device(d2.data_ptr(), d2.data_ptr(), n, z)
    assert np.array_equal(host(d2), want)
    d3 = dv.clone()
    gpu.batch_invert_device(d3.data_ptr(), n)
    assert np.array_equal(host(d3), P.batch_invert(v))


@pytest.mark.parametrize("n", [1 << 19, (1 << 19) + 1])
def test_scans_where_the_fused_form_ends_vs_oracle(gpu, torch, oracle, n):
    """2^19 elements leave 256 block totals, the most that every workgroup of the carry pass scans for itself (two launches); one element more leaves
    257, the first length whose block totals get a level of their own (four launches), and a last block of one element.  Every output against the
    big-integer oracle, inputs partly non-canonical.  The oracle takes about a second per scan of this length, so 2^19 + 1 is checked in full and 2^19
    in the suffix product and the opening."""
    full = n > 1 << 19
    v = noncanonical(oracle.random_scalars(0xF5ED + n, n), FR_MODULUS)
    z = oracle.random_scalars(0xF5EE + n, 1)[0]
    dv = dev(torch, v)
    out = torch.zeros_like(dv)
    for reverse, inclusive in ((True, False), (False, True)) if full else ((True, False),):
        gpu.product_scan_device(dv.data_ptr(), out.data_ptr(), n, reverse, inclusive)
        assert np.array_equal(host(out), P.product_scan(v, reverse, inclusive)), (n, reverse, inclusive)
    f = gpu.compute_kate_opening_coefficients_device(dv.data_ptr(), out.data_ptr(), n, z)
    want, wf = P.kate_opening(v, z)
    assert np.array_equal(host(out), want) and np.array_equal(f, wf)
    d2 = dv.clone()  # in place
    f2 = gpu.compute_kate_opening_coefficients_device(d2.data_ptr(), d2.data_ptr(), n, z)
    assert np.array_equal(host(d2), want) and np.array_equal(f2, wf)
    if full:
        assert np.array_equal(gpu.evaluate_device(dv.data_ptr(), n, z), P.evaluate(v, z))


@pytest.mark.parametrize("log2n", [2, 5, 10])
def test_domain_helpers_vs_oracle(gpu, torch, oracle, log2n):
    n = 1 << log2n
    for k in (1, 2, 4):
        l1 = torch.zeros((k * n, 4), dtype=torch.int64, device="cuda")
        gpu.compute_lagrange_polynomial_fft_device(l1.data_ptr(), n, k * n)
        assert np.array_equal(host(l1), P.lagrange_l1_fft(n, k * n)), (n, k)
        c = oracle.random_scalars(0xD1F + n + k, k * n)
        dc = dev(torch, c)
        gpu.divide_by_pseudo_vanishing_polynomial_device(dc.data_ptr(), n, k * n)
        assert np.array_equal(host(dc), P.divide_by_pseudo_vanishing(c, n, k * n)), (n, k)
    rng = np.random.default_rng(n)
    mapping = (rng.integers(0, n, size=n, dtype=np.uint32) + (rng.integers(0, 3, size=n, dtype=np.uint32) << np.uint32(30))).astype(np.uint32)
    dm = torch.from_numpy(mapping.view(np.int32)).cuda()
    out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    gpu.compute_permutation_lagrange_base_single_device(out.data_ptr(), dm.data_ptr(), n)
    assert np.array_equal(host(out), P.permutation_lagrange_base(mapping, n))


# ------------------------------------------------------------------ size-independent properties at BASELINE size ---------
@pytest.mark.parametrize("n", [1 << 20, (1 << 22) + 5, 1 << 23])
def test_helpers_properties_2_20(gpu, torch, oracle, n):
    """n = 2^20, and beyond 2^22 where the scan over the block totals is a three-phase scan of its own (round 4; 2^22 + 5: the inner scan has two
    workgroups, the second nearly empty): a^-1 * a = 1 everywhere; (X - z) W(X) + F(z) = F(X) checked at a random point through evaluate;
    inclusive prefix product's last element = exclusive suffix product's first * a_0; a prefix of the running product against the big-integer oracle"""
    v = oracle.random_scalars(0xB16, n)
    z, x = oracle.random_scalars(0xB17, 2)
    dv = dev(torch, v)
    inv = dv.clone()
    gpu.batch_invert_device(inv.data_ptr(), n)
    prod = torch.zeros_like(dv)
    gpu.mul_device(prod.data_ptr(), dv.data_ptr(), inv.data_ptr(), n)
    one = torch.from_numpy(P.mont([1]).view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert bool((prod == one).all())
    w = torch.zeros_like(dv)
    fz = gpu.compute_kate_opening_coefficients_device(dv.data_ptr(), w.data_ptr(), n, z)
    fx = P.plain(gpu.evaluate_device(dv.data_ptr(), n, x))[0]
    wx = P.plain(gpu.evaluate_device(w.data_ptr(), n, x))[0]
    zp, xp, fzp = P.plain(z)[0], P.plain(x)[0], P.plain(fz)[0]
    assert ((xp - zp) * wx + fzp) % FR_MODULUS == fx
    assert np.array_equal(fz, gpu.evaluate_device(dv.data_ptr(), n, z))
    pre, suf = torch.zeros_like(dv), torch.zeros_like(dv)
    gpu.product_scan_device(dv.data_ptr(), pre.data_ptr(), n, False, True)
    gpu.product_scan_device(dv.data_ptr(), suf.data_ptr(), n, True, False)
    total = P.plain(host(pre[n - 1:n]))[0]
    assert total == P.plain(host(suf[0:1]))[0] * P.plain(v[0:1])[0] % FR_MODULUS
    # chunk-wise check of the whole-vector product against the big-integer oracle on a sub-range
    m = 3000
    assert P.plain(host(pre[m - 1:m]))[0] == P.plain(P.product_scan(v[:m], False, True)[m - 1:m])[0]
    # the recurrences themselves where carries cross a level: run, workgroup (2048), the inner scan's workgroup (2048 x 2048) and ragged positions
    hp, hs, hw = host(pre), host(suf), host(w)
    ks = sorted({k for k in (1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, (1 << 20) - 1, 1 << 20, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 22) + 4,
                             3 * (1 << 21) + 123, n - 2, n - 1) if 1 <= k < n})
    pv, pp, ps, pw = P.plain(v[ks]), P.plain(hp[ks]), P.plain(hs[ks]), P.plain(hw[ks])
    pp1, ps1, pw1 = P.plain(hp[[k - 1 for k in ks]]), P.plain(hs[[k - 1 for k in ks]]), P.plain(hw[[k - 1 for k in ks]])
    for i, k in enumerate(ks):
        assert pp[i] == pp1[i] * pv[i] % FR_MODULUS, ("prefix", n, k)           # inclusive prefix: pre[k] = pre[k-1] v[k]
        assert ps1[i] == ps[i] * pv[i] % FR_MODULUS, ("suffix", n, k)           # exclusive suffix: suf[k-1] = suf[k] v[k]
        assert pw1[i] == (pv[i] + zp * pw[i]) % FR_MODULUS, ("kate", n, k)      # W[k-1] = F[k] + z W[k]


# ------------------------------------------------------------------ the resident prover ----------------------------------
SECRET_RAW = 0x0123456789ABCDEF_0F1E2D3C4B5A6978_FEDCBA9876543210_0123456789ABCDEF  # oracle/plonk_driver.cpp secret(), limbs 3..0


@pytest.fixture(scope="module")
def srs65536(gpu):
    x_mont = P.mont([SECRET_RAW % FR_MODULUS])[0]
    return gpu.srs_generate(x_mont, 65536)


@pytest.fixture(scope="module")
def srs_for(gpu, srs65536):
    """SRS handle holding at least n points of the same synthetic SRS x^i G"""
    made = {}

    def get(n):
        if n <= 65536:
            return srs65536
        if n not in made:
            made[n] = gpu.srs_generate(P.mont([SECRET_RAW % FR_MODULUS])[0], n)
        return made[n]
    yield get
    for h in made.values():
        gpu.srs_release(h)


@pytest.mark.parametrize("gates", [32, 1024, 16384, 65536, 262144, 1048576, 2097152])
def test_resident_prover_proof_is_byte_identical(gpu, srs_for, golden, gates):
    """BASELINE config 5, natively: the bench_plonk.cpp add/mul-chain circuit built by the StandardComposer mirror (its state is
    pinned against the reference composer in tests/test_plonk_host.py), proved by bbgpu_plonk_construct_proof with all
    polynomials resident, against the proof the reference's all-CPU prover made for the same circuit, witnesses and SRS.
    2^18 and 2^20 gates use the same fixtures; the reference needed 3.7 s / 13.6 s for them on 8 cores (tools/gen_plonk_golden.py).
    2^21 gates: the 4n = 2^23 transforms take the three-pass NTT and the 2^21-point commitments run without window tables."""
    from barretenberg_amd.plonk import Prover, bench_circuit, proof_lines
    tr = golden("plonk_trace.json")
    state = bench_circuit(gates, int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)).preprocess()
    prover = Prover(gpu, state, srs_for(state["n"]))
    try:
        want = golden("plonk_proofs.json")["proofs"][str(gates)]
        proof = prover.construct_proof()
        got = proof_lines(state["n"], proof)
        ch = prover.challenges()
        for name in ("gamma", "beta", "alpha", "z", "nu"):
            assert hx(ch[name])[0] == tr["challenges"][str(gates)][name], name
        assert got == want[:26]
        # the verification key waffle::preprocess() derives (SIGMA_1..3, Q_M..Q_C commitments) equals the reference's
        if str(gates) in tr["verification_keys"]:
            from barretenberg_amd.plonk import VK_POINTS, hex4
            from oracle.pyoracle import Oracle
            vk = prover.preprocess()
            ref = {ln.split()[0]: ln.split()[1] for ln in tr["verification_keys"][str(gates)][1:]}
            for k in VK_POINTS:
                if int(vk[k][7]) >> 63:
                    # commitment to the zero polynomial (q_c of this circuit): the point at infinity.  The reference pushes its infinity
                    # through jacobian_to_affine and stores an off-curve pair, which its verifier then skips
                    # (`if (g1::on_curve(instance[i]))`, arithmetic_widget.cpp:190-230) -- nothing to compare but that
                    rp = np.array([int(ref[k + c][16 * (3 - j):16 * (4 - j)], 16) for c in (".x", ".y") for j in range(4)], dtype=np.uint64)
                    assert not Oracle().g1_on_curve(rp), k
                    continue
                assert hex4(vk[k][0:4]) == ref[k + ".x"] and hex4(vk[k][4:8]) == ref[k + ".y"], k
        # proving again (cached circuit state, same witness) and after re-uploading the witness gives the same bytes
        assert np.array_equal(prover.construct_proof(), proof)
        prover.set_witness(state["w_l"], state["w_r"], state["w_o"])
        assert np.array_equal(prover.construct_proof(), proof)
        # the reference's own Verifier accepts it (when the reference build travelled with the repo)
        exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
        if gates <= 65536 and os.path.exists(exe) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "transcript.dat")):
            r = subprocess.run([exe, "verify", str(gates)], input="\n".join(got) + "\n", cwd=ROOT, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, OMP_NUM_THREADS="16"))
            assert r.returncode == 0 and r.stdout.strip() == "verified 1", (r.stdout, r.stderr[-500:])
    finally:
        prover.destroy()


def test_commitments_at_infinity(gpu, srs65536, golden):
    """A commitment that is the point at infinity.  What the reference does is pinned by tests/golden/infinity_commitments.json
    (tools/gen_infinity_golden.py, CPU half of the check in tests/test_plonk_host.py): the flag -- bit 63 of y.data[3] -- is always set, every
    other bit of the pair is run-dependent garbage that even reaches its Fiat-Shamir hash.  This library returns the CLEAN encoding (x = 0,
    y = the flag alone) at every boundary, which is a member of the same class; checked here:
      * bbgpu_msm_g1 of all-zero scalars -> the clean encoding;
      * the resident prover on the zero-wire circuit: W_R and W_O are the clean encoding, W_L equals the reference's (it precedes the
        hash), and the REFERENCE's own Verifier accepts the proof;
      * the reference's unmodified Prover linked on the shim emits flagged points for the same circuit and its proof verifies."""
    from barretenberg_amd.plonk import Prover, proof_lines, zero_wire_circuit
    fx = golden("infinity_commitments.json")
    flag = 1 << 63
    # boundary MSM
    n = 4096
    table = np.zeros((2 * n, 8), dtype=np.uint64)
    h, table = gpu.srs_generate(np.array([5, 6, 7, 8], dtype=np.uint64), n, True)
    out = gpu.pippenger(np.zeros((n, 4), dtype=np.uint64), table, n)
    assert [int(v) for v in out[:8]] == [0, 0, 0, 0, 0, 0, 0, flag]
    gpu.srs_release(h)
    # resident prover
    a0 = 0x0777777788888888555555556666666633333333444444441111111122222222
    state = zero_wire_circuit(32, a0).preprocess()
    assert state["n"] == fx["n"]
    prover = Prover(gpu, state, srs65536)
    try:
        proof = prover.construct_proof()
        lines = proof_lines(state["n"], proof)
        got = dict(ln.split() for ln in lines[1:])
        for k in ("W_R", "W_O"):
            assert got[k + ".x"] == "0" * 64 and got[k + ".y"] == "8" + "0" * 63, (k, got[k + ".x"], got[k + ".y"])
        for t in ("1", "4", "8"):
            assert got["W_L.x"] == fx["proof_zerowire_circuit"][t]["W_L.x"] and got["W_L.y"] == fx["proof_zerowire_circuit"][t]["W_L.y"]
        exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
        if not os.path.exists(exe):
            pytest.fail("oracle/_ref/plonk_cpu is missing: the reference's Verifier is the judge of this test")
        r = subprocess.run([exe, "verify", "32"], input="\n".join(lines) + "\n", cwd=ROOT, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, OMP_NUM_THREADS="4", BB_CIRCUIT="zerowire", BBGPU_SHIM_STRICT="1"))
        assert r.returncode == 0 and r.stdout.strip() == "verified 1", (r.stdout, r.stderr[-500:])
    finally:
        prover.destroy()
    # the reference prover on the shim
    exe = os.path.join(ROOT, "oracle", "_ref", "plonk_gpu")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/plonk_gpu is missing")
    r = subprocess.run([exe, "trace", "32"], cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="4", BB_CIRCUIT="zerowire", BBGPU_SHIM_STRICT="1"))
    shim = dict(ln.split() for ln in r.stdout.strip().split("\n") if len(ln.split()) == 2)
    assert shim.get("verified") == "1", (r.stdout[-400:], r.stderr[-400:])
    for k in ("W_R", "W_O"):
        assert int(shim[k + ".y"][:16], 16) >> 63 == 1, (k, shim[k + ".y"])
    assert shim["W_L.x"] == got["W_L.x"] and shim["W_L.y"] == got["W_L.y"]


def test_resident_prover_rejects_bad_input(gpu, srs65536):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.plonk import Prover, bench_circuit
    state = bench_circuit(32, 3, 5).preprocess()
    bad = dict(state, n=24)
    for k in bad:
        if k != "n":
            bad[k] = bad[k][:24]
    with pytest.raises(BbGpuError):
        Prover(gpu, bad, srs65536)
    with pytest.raises(BbGpuError):
        Prover(gpu, state, 12345)


def test_resident_prover_on_a_transcript_file(gpu, golden, tmp_path):
    """the SRS path a real deployment takes: an ignition-format transcript file (io.hpp:36-182) read by bbgpu_transcript_read_g1,
    registered (uploaded + window tables) and used by the resident prover -- same proof bytes as with the device-generated SRS.
    The file is written here from the synthetic SRS in the format's own terms (limb 0 first, limbs big-endian, plain form)."""
    from barretenberg_amd.plonk import Prover, bench_circuit, proof_lines
    from oracle.pyoracle import FQ, Oracle
    O = Oracle()
    n = 1024
    srs = O.make_srs(P.mont([SECRET_RAW % FR_MODULUS])[0], n)
    path = str(tmp_path / "transcript.dat")
    with open(path, "wb") as fh:
        for v in (0, 1, n - 1, 2, n - 1, 2, 0):
            fh.write(int(v).to_bytes(4, "big"))
        for i in range(1, n):
            for c in (srs[i][0:4], srs[i][4:8]):
                for limb in O.from_mont(FQ, c):
                    fh.write(int(limb).to_bytes(8, "big"))
        fh.write(bytes(256 + 64))
    table = gpu.read_transcript(path, n)
    h = gpu.srs_register(table)
    tr = golden("plonk_trace.json")
    for gates in (32, 1024):
        state = bench_circuit(gates, int(tr["witness_a0"], 16), int(tr["witness_b0"], 16)).preprocess()
        prover = Prover(gpu, state, h)
        try:
            assert proof_lines(state["n"], prover.construct_proof()) == golden("plonk_proofs.json")["proofs"][str(gates)][:26]
        finally:
            prover.destroy()
    gpu.srs_release(h)


def test_product_written_transcript_is_read_by_the_reference(gpu, golden, tmp_path):
    """SURVEY 8f #3 closed: the PRODUCT creates the file BASELINE configs 2 / 5 name -- bbgpu_srs_generate (device) + bbgpu_transcript_write
    (G1 from the generated table, G2 half from the secret) -- and the reference's own io::read_transcript, Prover and Verifier
    (oracle/_ref/plonk_cpu, all-CPU reference build) take it: same golden proof bytes, pairing check passes."""
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
    if not os.path.exists(exe):
        pytest.fail("oracle/_ref/plonk_cpu is missing: the reference build must travel with the repo (built by __graft_entry__.build() in the build container)")
    n = 4096
    x = P.mont([SECRET_RAW % FR_MODULUS])[0]
    h, table = gpu.srs_generate(x, n, want_host_table=True)
    gpu.srs_release(h)
    d = tmp_path / "oracle" / "_ref"   # the reference build reads the cwd-relative path oracle/_ref/transcript.dat (oracle/Makefile)
    d.mkdir(parents=True)
    gpu.write_transcript(str(d / "transcript.dat"), table, n, x)
    assert np.array_equal(gpu.read_transcript(str(d / "transcript.dat"), n), table)
    for gates in (32, 1024):
        r = subprocess.run([exe, "prove", str(gates)], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert any(l.startswith("verified 1") for l in lines), lines[-3:]
        gold = golden("plonk_proofs.json")["proofs"][str(gates)][:26]
        assert [l for l in lines if l.split()[0] in {g.split()[0] for g in gold}][:26] == gold


@pytest.mark.parametrize("gates", [2, 6, 14, 64, 4096])
def test_resident_prover_with_bool_widget(gpu, srs65536, golden, gates):
    """second widget of the chain: a BoolComposer circuit (arithmetic + bool widget, bool_widget.cpp) -- proof bytes, all five challenges and
    the verification key (11 commitments) equal the reference's; its Verifier accepts the proof.  gates = 2, 6, 14 are circuits of
    n = 4, 8, 16: the smallest proofs the reference's own tests make (test_verifier.cpp:105-122) -- 4-point MSMs, 4/8/16-point transforms."""
    from barretenberg_amd.plonk import VK_POINTS_BOOL, Prover, bool_circuit, hex4, proof_lines
    from oracle.pyoracle import Oracle
    fx = golden("plonk_trace.json")["bool"]
    state = bool_circuit(gates).preprocess()
    prover = Prover(gpu, state, srs65536)
    try:
        proof = prover.construct_proof()
        got = proof_lines(state["n"], proof)
        ch = prover.challenges()
        for name in ("gamma", "beta", "alpha", "z", "nu"):
            assert hx(ch[name])[0] == fx["challenges"][str(gates)][name], name
        assert got == fx["proofs"][str(gates)][:26]
        vk = prover.preprocess()
        ref = {ln.split()[0]: ln.split()[1] for ln in fx["verification_keys"][str(gates)][1:]}
        for k in VK_POINTS_BOOL:
            if int(vk[k][7]) >> 63:  # commitment to a zero selector (no boolean output wires here): see the arithmetic-widget test
                rp = np.array([int(ref[k + c][16 * (3 - j):16 * (4 - j)], 16) for c in (".x", ".y") for j in range(4)], dtype=np.uint64)
                assert not Oracle().g1_on_curve(rp), k
                continue
            assert hex4(vk[k][0:4]) == ref[k + ".x"] and hex4(vk[k][4:8]) == ref[k + ".y"], k
        assert np.array_equal(prover.construct_proof(), proof)
        exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
        if os.path.exists(exe) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "transcript.dat")):
            r = subprocess.run([exe, "verify", str(gates)], input="\n".join(got) + "\n", cwd=ROOT, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, OMP_NUM_THREADS="16", BB_CIRCUIT="bool"))
            assert r.returncode == 0 and r.stdout.strip() == "verified 1", (r.stdout, r.stderr[-500:])
    finally:
        prover.destroy()


MIMC_X0 = 0x0777777788888888555555556666666633333333444444441111111122222222
MIMC_K = 0x0ABCDEFABCDEFABC1234123412341234DDDDEEEEFFFF00009999AAAABBBBCCCC


@pytest.mark.parametrize("gates", [3, 6, 30, 93, 4094])
def test_resident_prover_with_mimc_widget(gpu, srs65536, golden, gates):
    """third widget: a MiMCComposer circuit (arithmetic + MiMC widget, mimc_widget.cpp) -- a chain of x <- (x + k + c_i)^7 rounds, whose
    identity reads w_o at the NEXT row, so the proof carries w_o(z*omega) and q_mimc_coefficient(z) as well.  Proof bytes (28 lines), all five
    challenges and the verification key (10 commitments) equal the reference's; its Verifier accepts the proof."""
    from barretenberg_amd.plonk import VK_POINTS_MIMC, Prover, hex4, mimc_circuit, proof_lines
    from oracle.pyoracle import Oracle
    fx = golden("plonk_trace.json")["mimc"]
    state = mimc_circuit(gates, MIMC_X0, MIMC_K).preprocess()
    prover = Prover(gpu, state, srs65536)
    try:
        proof = prover.construct_proof()
        got = proof_lines(state["n"], proof, mimc=True)
        ch = prover.challenges()
        for name in ("gamma", "beta", "alpha", "z", "nu"):
            assert hx(ch[name])[0] == fx["challenges"][str(gates)][name], name
        assert got == fx["proofs"][str(gates)][:28]
        vk = prover.preprocess()
        ref = {ln.split()[0]: ln.split()[1] for ln in fx["verification_keys"][str(gates)][1:]}
        for k in VK_POINTS_MIMC:
            if int(vk[k][7]) >> 63:  # commitment to a zero selector: see the arithmetic-widget test
                rp = np.array([int(ref[k + c][16 * (3 - j):16 * (4 - j)], 16) for c in (".x", ".y") for j in range(4)], dtype=np.uint64)
                assert not Oracle().g1_on_curve(rp), k
                continue
            assert hex4(vk[k][0:4]) == ref[k + ".x"] and hex4(vk[k][4:8]) == ref[k + ".y"], k
        assert np.array_equal(prover.construct_proof(), proof)
        exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
        if os.path.exists(exe) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "transcript.dat")):
            r = subprocess.run([exe, "verify", str(gates)], input="\n".join(got) + "\n", cwd=ROOT, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, OMP_NUM_THREADS="16", BB_CIRCUIT="mimc"))
            assert r.returncode == 0 and r.stdout.strip() == "verified 1", (r.stdout, r.stderr[-500:])
    finally:
        prover.destroy()


def _extended_state(gates):
    """the waffle::Prover input state the reference's ExtendedComposer produced for the fixture circuit (data, tools/gen_plonk_golden.py)"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "plonk_extended_state.npz"))
    st = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("%d/" % gates)}
    st["n"] = int(st["n"][0])
    return st


@pytest.mark.parametrize("gates", [8, 32, 100, 160])
def test_resident_prover_with_sequential_and_bool_widgets(gpu, srs65536, golden, gates):
    """the ExtendedComposer's widget chain -- arithmetic, sequential (q_o_next * w_o at the next row, sequential_widget.cpp), bool -- on the
    resident prover.  The composer's gate folding is not mirrored: the Prover input state the reference composer produced is the fixture.
    Proof bytes (27 lines, with w_o_shifted_eval), all five challenges and the verification key (12 commitments) equal the reference's; its
    Verifier accepts the proof."""
    from barretenberg_amd.plonk import VK_POINTS_EXTENDED, Prover, hex4, proof_lines
    from oracle.pyoracle import Oracle
    fx = golden("plonk_trace.json")["extended"]
    state = _extended_state(gates)
    assert any(int(v) for v in state["q_o_next"].ravel()) and any(int(v) for v in state["q_br"].ravel())  # both extra widgets are exercised
    prover = Prover(gpu, state, srs65536)
    try:
        proof = prover.construct_proof()
        got = proof_lines(state["n"], proof, sequential=True)
        ch = prover.challenges()
        for name in ("gamma", "beta", "alpha", "z", "nu"):
            assert hx(ch[name])[0] == fx["challenges"][str(gates)][name], name
        assert got == fx["proofs"][str(gates)][:27]
        vk = prover.preprocess()
        ref = {ln.split()[0]: ln.split()[1] for ln in fx["verification_keys"][str(gates)][1:]}
        for k in VK_POINTS_EXTENDED:
            if int(vk[k][7]) >> 63:  # commitment to a zero selector: see the arithmetic-widget test
                rp = np.array([int(ref[k + c][16 * (3 - j):16 * (4 - j)], 16) for c in (".x", ".y") for j in range(4)], dtype=np.uint64)
                assert not Oracle().g1_on_curve(rp), k
                continue
            assert hex4(vk[k][0:4]) == ref[k + ".x"] and hex4(vk[k][4:8]) == ref[k + ".y"], k
        assert np.array_equal(prover.construct_proof(), proof)
        exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
        if os.path.exists(exe) and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "transcript.dat")):
            r = subprocess.run([exe, "verify", str(gates)], input="\n".join(got) + "\n", cwd=ROOT, capture_output=True, text=True, timeout=300,
                               env=dict(os.environ, OMP_NUM_THREADS="16", BB_CIRCUIT="extended"))
            assert r.returncode == 0 and r.stdout.strip() == "verified 1", (r.stdout, r.stderr[-500:])
    finally:
        prover.destroy()
