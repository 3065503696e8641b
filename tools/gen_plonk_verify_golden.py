#!/usr/bin/env python3
"""tests/golden/plonk_verify.json: what the REFERENCE's Verifier::verify_proof says about honest and tampered proofs.
Base proofs come from tests/golden/plonk_proofs.json / plonk_trace.json (standard, bool, MiMC, extended circuits) and, for the zero-wire circuit
whose W_R and W_O are the point at infinity, from a fresh `BB_CIRCUIT=zerowire plonk_cpu trace 32` (tests/golden/infinity_commitments.json: the
reference has no reproducible bytes for it).  Every row is fed to `oracle/_ref/plonk_cpu verify <gates>` (the reference's unmodified Verifier,
compiled in place by oracle/Makefile; driver oracle/plonk_driver.cpp) and its verdict recorded.  The generator ASSERTS that the status rule of
include/bbgpu.h (BAD_POINT / ZERO_EVAL, evaluated here on Python integers) never flags a proof the reference accepts, and that every tamper gets the
verdict its construction implies; if one does not, the rule is wrong, not the fixture.
Valid proofs of OTHER WITNESSES: the driver's witnesses are fixed and there is no prover on the CPU, so those rows are proofs the batch prover made
on a GPU (`python tools/gen_plonk_verify_golden.py --make-other-witness FILE` on an MI355X writes four of the 32-gate bench circuit); their verdict
is, like every row's, the reference's.  `--other-witness FILE` takes them in; without it the rows of the existing fixture are kept (and asked again).
Run in the build container (needs oracle/_ref):  python tools/gen_plonk_verify_golden.py [--other-witness FILE]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from barretenberg_amd import BbGpu  # noqa: E402
from barretenberg_amd.plonk import PROOF_EVALS, PROOF_EVALS_WIDGET, PROOF_POINTS, hex4, proof_words  # noqa: E402

EXE = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
P = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b97091 << 64 | 0x43e1f593f0000001
MONT = 1 << 256
WIDGETS = {"standard": 0, "bool": 1, "mimc": 2, "extended": 4 | 1, "zerowire": 0}
EVALS = list(PROOF_EVALS) + list(PROOF_EVALS_WIDGET)
INF_Y = 1 << 255


def get(words, i):
    return sum(int(words[4 * i + k]) << (64 * k) for k in range(4))


def put(words, i, v):
    for k in range(4):
        words[4 * i + k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF


def on_curve(words, point):
    """the rule's curve test: flag clear and y^2 = x^3 + 3 on the residues"""
    x, y = get(words, 2 * point), get(words, 2 * point + 1)
    if y >> 255:
        return None  # the infinity flag
    rinv = pow(MONT, -1, P)
    x, y = x * rinv % P, y * rinv % P
    return (y * y - x * x * x - 3) % P == 0


def rule_status(words):
    st = 0
    for i, name in enumerate(PROOF_POINTS):
        oc = on_curve(words, i)
        if oc is None:
            st |= 1 if name in ("Z_1", "T_LO", "PI_Z") else 0
        elif not oc:
            st |= 1
    for name in ("sigma_1_eval", "sigma_2_eval", "linear_eval"):
        if get(words, 18 + EVALS.index(name)) == 0:
            st |= 2
    return st


def double_point(words, point):
    rinv = pow(MONT, -1, P)
    x, y = get(words, 2 * point) * rinv % P, get(words, 2 * point + 1) * rinv % P
    lam = 3 * x * x * pow(2 * y, -1, P) % P
    x3 = (lam * lam - 2 * x) % P
    y3 = (lam * (x - x3) - y) % P
    put(words, 2 * point, x3 * MONT % P)
    put(words, 2 * point + 1, y3 * MONT % P)


def lines_of(n, words, kind):
    out = ["n %d" % n]
    for i, name in enumerate(PROOF_POINTS):
        out += ["%s.x %s" % (name, hex4(words[8 * i:8 * i + 4])), "%s.y %s" % (name, hex4(words[8 * i + 4:8 * i + 8]))]
    for i, name in enumerate(PROOF_EVALS):
        out.append("%s %s" % (name, hex4(words[72 + 4 * i:76 + 4 * i])))
    if kind in ("mimc", "extended"):
        out.append("w_o_shifted_eval %s" % hex4(words[108:112]))
    if kind == "mimc":
        out.append("q_mimc_coefficient_eval %s" % hex4(words[116:120]))
    return out


def env_of(kind):
    return dict(os.environ) if kind == "standard" else dict(os.environ, BB_CIRCUIT=kind)


def reference_verdict(kind, gates, n, words):
    r = subprocess.run([EXE, "verify", str(gates)], cwd=ROOT, input="\n".join(lines_of(n, words, kind)) + "\n", capture_output=True, text=True,
                       env=env_of(kind), check=False)
    last = [ln for ln in r.stdout.strip().split("\n") if ln.startswith("verified")]
    assert last and r.returncode in (0, 2), (kind, gates, r.returncode, r.stdout, r.stderr)
    return int(last[-1].split()[1])


def tampers(full):
    """(name, function on the words, verdict the construction implies) -- the full matrix, or a handful"""
    out = [("none", lambda w: None, 1)]

    def neg(i):
        return lambda w: put(w, 2 * i + 1, (P - get(w, 2 * i + 1)) % P)

    def off(i):
        return lambda w: put(w, 2 * i, (get(w, 2 * i) + 1) % P)

    def inf(i):
        def f(w):
            put(w, 2 * i, 0)
            put(w, 2 * i + 1, INF_Y)
        return f

    def ev_plus_one(e):
        return lambda w: put(w, 18 + e, (get(w, 18 + e) + MONT % R_MOD) % R_MOD)

    if full:
        for i, name in enumerate(PROOF_POINTS):
            out.append(("neg_" + name, neg(i), 0))
        for i, name in enumerate(PROOF_POINTS):
            out.append(("double_" + name, (lambda i: lambda w: double_point(w, i))(i), 0))
        for e, name in enumerate(EVALS):
            # the standard circuit's verifier never reads the five widget evaluations: a change there changes nothing
            out.append(("plus_one_" + name, ev_plus_one(e), 0 if e < 7 else 1))
    else:
        out += [("neg_Z_1", neg(3), 0), ("double_PI_Z_OMEGA", lambda w: double_point(w, 8), 0), ("plus_one_linear_eval", ev_plus_one(6), 0)]
    out += [("infinity_W_L", inf(0), 0), ("infinity_T_HI", inf(6), 0), ("off_curve_PI_Z", off(7), 0), ("off_curve_W_R", off(1), 0),
            ("sigma_1_eval_zero", lambda w: put(w, 18 + 3, 0), 0), ("sigma_1_eval_r", lambda w: put(w, 18 + 3, R_MOD), 0)]
    return out


def make_other_witness(path):
    """on a GPU: four proofs of the 32-gate bench circuit for witnesses of our own choosing, by ONE call of the batch prover"""
    from oracle.pyoracle import FR_MODULUS
    from barretenberg_amd.plonk import Prover, bench_circuit, to_montgomery_limbs
    secret = 0x0123456789ABCDEF0F1E2D3C4B5A6978FEDCBA98765432100123456789ABCDEF  # the x of oracle/_ref/transcript.dat
    G = BbGpu(device=0)
    hs = G.srs_generate(to_montgomery_limbs([secret % FR_MODULUS])[0], 1024)
    states = [bench_circuit(32, 3 + 5 * k, 7 + 11 * k).preprocess() for k in range(4)]
    prover = Prover(G, states[0], hs)
    proofs = prover.construct_proofs([(s["w_l"], s["w_r"], s["w_o"]) for s in states])
    prover.destroy()
    G.shutdown()
    with open(path, "w") as fh:
        json.dump(["".join("%016x" % int(v) for v in p) for p in proofs], fh)
    print("wrote %d proofs to %s" % (len(proofs), path))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--make-other-witness":
        return make_other_witness(sys.argv[2])
    G = BbGpu(init=False)
    proofs = json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_proofs.json")))["proofs"]
    trace = json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_trace.json")))
    g2_x = G.transcript_read_g2(os.path.join(ROOT, "oracle", "_ref", "transcript.dat"))
    out = {"source": "oracle/_ref/plonk_cpu verify <gates> (the reference's own Verifier::verify_proof; see tools/gen_plonk_verify_golden.py)",
           "g2_x": ["%016x" % int(v) for v in g2_x], "circuits": {}, "rows": []}
    zero_lines = subprocess.run([EXE, "trace", "32"], cwd=ROOT, capture_output=True, text=True, check=True, env=env_of("zerowire")).stdout.strip().split("\n")
    bases = [("standard", 32, proofs["32"], True), ("standard", 1024, proofs["1024"], False), ("bool", 14, trace["bool"]["proofs"]["14"], False),
             ("mimc", 30, trace["mimc"]["proofs"]["30"], False), ("extended", 32, trace["extended"]["proofs"]["32"], False),
             ("zerowire", 32, [ln for ln in zero_lines if len(ln.split()) == 2], False)]
    honest = {}
    for kind, gates, lines, full in bases:
        n, words = proof_words(lines)
        key = "%s/%d" % (kind, gates)
        honest[key] = (n, words)
        vk = subprocess.run([EXE, "vk", str(gates)], cwd=ROOT, capture_output=True, text=True, check=True, env=env_of(kind)).stdout.strip().split("\n")
        vk = [ln for ln in vk if len(ln.split()) == 2 and ln.split()[0] != "n"]
        if kind != "zerowire":
            known = (trace if kind == "standard" else trace[kind])["verification_keys"][str(gates)]
            assert [ln for ln in known if ln.split()[0] != "n"] == vk, key
        out["circuits"][key] = {"kind": kind, "gates": gates, "n": n, "widgets": WIDGETS[kind], "vk": [ln.split()[1] for ln in vk]}
        for name, fn, implied in tampers(full) if kind != "zerowire" else [("none", lambda w: None, 1)]:
            w = words.copy()
            fn(w)
            verdict = reference_verdict(kind, gates, n, w)
            status = rule_status(w)
            assert verdict == implied, (key, name, verdict)
            assert not (status and verdict), (key, name, status)
            out["rows"].append({"circuit": key, "tamper": name, "rule_status": status, "reference_verdict": verdict, "proof": "".join("%016x" % int(v) for v in w)})
            print(key, name, "status", status, "verdict", verdict)
    # a valid proof of a DIFFERENT circuit of the same n: the extended circuit's proof before the standard circuit's verifier (both n = 32)
    n_x, w_x = honest["extended/32"]
    assert n_x == honest["standard/32"][0]
    verdict = reference_verdict("standard", 32, n_x, w_x)
    assert verdict == 0 and rule_status(w_x) == 0
    out["rows"].append({"circuit": "standard/32", "tamper": "proof_of_extended_32", "rule_status": 0, "reference_verdict": verdict,
                        "proof": "".join("%016x" % int(v) for v in w_x)})
    # valid proofs of other witnesses of the standard circuit (made by the batch prover; see the module text)
    path = os.path.join(ROOT, "tests", "golden", "plonk_verify.json")
    if len(sys.argv) == 3 and sys.argv[1] == "--other-witness":
        others = json.load(open(sys.argv[2]))
    else:
        others = [r["proof"] for r in json.load(open(path))["rows"] if r["tamper"].startswith("other_witness_")] if os.path.exists(path) else []
    for k, hexproof in enumerate(others):
        w = np.array([int(hexproof[16 * i:16 * i + 16], 16) for i in range(120)], dtype=np.uint64)
        assert not np.array_equal(w, honest["standard/32"][1])
        verdict = reference_verdict("standard", 32, 32, w)
        assert verdict == 1 and rule_status(w) == 0, (k, verdict)
        out["rows"].append({"circuit": "standard/32", "tamper": "other_witness_%d" % k, "rule_status": 0, "reference_verdict": verdict, "proof": hexproof})
        print("standard/32 other_witness_%d status 0 verdict %d" % (k, verdict))
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
    print("wrote tests/golden/plonk_verify.json: %d rows" % len(out["rows"]))


if __name__ == "__main__":
    main()
