"""What verifying PLONK proofs costs on one MI355X (profiles/plonk_verify.txt is this tool's output), one process on one box, the legs alternating
inside every repetition.  Proofs: the batch prover's, of the bench circuit at `--gates` gates (the gate count only changes the k squarings of z^n),
tiled to the count.  Per count, wall milliseconds PER PROOF (median / min of `--reps` rounds after one warm round) of
  gpu        bbgpu_plonk_verify_batch, fixed seed, no LOCATE, and its split by bbgpu_plonk_verify_last_timing (medians): upload + k_verify_terms +
             status read-back | k_verify_fold | the two MSMs | the host tail (one product of two pairings, normalisations)
  host       bbgpu_host_plonk_verify_batch, the host twin (counts up to --host-max)
and once, as the yardstick, the reference's Verifier::verify_proof through oracle/_ref/plonk_cpu: the driver has no timer around verify_proof, so it
is the PAIRED DIFFERENCE of two process walls at 32 gates, `plonk_cpu verify 32` (circuit, preprocess, verify_proof) minus `plonk_cpu vk 32` (circuit,
preprocess), median and quartiles over alternating pairs -- at 2^16 gates both walls are seconds of composer and preprocess and the difference drowns;
the printed line says what it is.  Usage: python tools/plonk_verify_bench.py [--gates 65536] [--counts 16,256,4096,16384] [--reps 7]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SECRET = 0x0123456789ABCDEF0F1E2D3C4B5A6978FEDCBA98765432100123456789ABCDEF  # the x of oracle/_ref/transcript.dat


def med_min(ts):
    return statistics.median(ts), min(ts)


def reference_ms(runs):
    """-> (median, lower quartile, upper quartile) of the PAIRED differences `verify 32` - `vk 32`, and the two medians"""
    exe = os.path.join(ROOT, "oracle", "_ref", "plonk_cpu")
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "plonk_proofs.json")))["proofs"]["32"]
    text = "\n".join(gold[:26]) + "\n"
    env = dict(os.environ, OMP_NUM_THREADS="1")
    t_verify, t_vk = [], []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        r = subprocess.run([exe, "verify", "32"], cwd=ROOT, input=text, capture_output=True, text=True, env=env)
        t1 = time.perf_counter()
        subprocess.run([exe, "vk", "32"], cwd=ROOT, capture_output=True, text=True, env=env)
        t2 = time.perf_counter()
        assert "verified 1" in r.stdout, r.stdout
        t_verify.append((t1 - t0) * 1e3)
        t_vk.append((t2 - t1) * 1e3)
    diff = sorted(a - b for a, b in zip(t_verify[1:], t_vk[1:]))
    q = statistics.quantiles(diff, n=4)
    return (statistics.median(diff), q[0], q[2]), statistics.median(t_verify[1:]), statistics.median(t_vk[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gates", type=int, default=65536)
    ap.add_argument("--counts", default="16,256,4096,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-max", type=int, default=4096)
    ap.add_argument("--reference-runs", type=int, default=41)
    args = ap.parse_args()
    from oracle.pyoracle import FR_MODULUS
    from barretenberg_amd import BbGpu
    from barretenberg_amd.plonk import Prover, Verifier, bench_circuit, to_montgomery_limbs
    G = BbGpu(device=0)
    g2_x = G.transcript_read_g2(os.path.join(ROOT, "oracle", "_ref", "transcript.dat"))
    hs = G.srs_generate(to_montgomery_limbs([SECRET % FR_MODULUS])[0], max(args.gates, 1024))
    states = [bench_circuit(args.gates, 3 + 5 * k, 7 + 11 * k).preprocess() for k in range(2)]
    P = Prover(G, states[0], hs)
    V = Verifier.from_prover(P, g2_x)
    base = P.construct_proofs([(s["w_l"], s["w_r"], s["w_o"]) for s in states] * 8)
    seed = np.arange(1, 5, dtype=np.uint64)
    print("# %s; %d gates (n = %d); wall ms PER PROOF, median / min of %d alternating rounds" % (G.version(), args.gates, V.n, args.reps))
    for count in [int(c) for c in args.counts.split(",")]:
        proofs = np.ascontiguousarray(base[np.arange(count) % base.shape[0]])
        with_host = count <= args.host_max
        gpu, host, split = [], [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            r = V.verify(proofs, seed)
            t1 = time.perf_counter()
            assert r.ok, r.as_dict()
            if rep:
                gpu.append((t1 - t0) * 1e3 / count)
                split.append(G.plonk_verify_last_timing())
            if with_host:
                t0 = time.perf_counter()
                h = V.verify(proofs, seed, host=True)
                t1 = time.perf_counter()
                assert h.ok and list(h.a) == list(r.a) and list(h.b) == list(r.b)
                if rep:
                    host.append((t1 - t0) * 1e3 / count)
        sp = {k: statistics.median(s[k] for s in split) for k in split[0]}
        line = "count %6d  gpu %9.5f / %9.5f" % ((count,) + med_min(gpu))
        line += "  host %9.5f / %9.5f" % med_min(host) if with_host else "  host         - /         -"
        line += "  | one gpu call %8.3f ms = terms %7.3f + fold %6.3f + two MSMs %7.3f + host tail %6.3f" % (
            sp["total_ms"], sp["terms_ms"], sp["fold_ms"], sp["msm_ms"], sp["host_tail_ms"])
        print(line, flush=True)
    V.destroy()
    P.destroy()
    G.srs_release(hs)
    G.shutdown()
    (d, d_lo, d_hi), v, k = reference_ms(args.reference_runs)
    print("reference, Verifier::verify_proof of ONE proof: %.3f ms (quartiles %.3f .. %.3f) -- NOT the same proofs and NOT a timer around the call: the"
          " paired difference of two process walls of oracle/_ref/plonk_cpu at 32 gates and one thread, `verify 32` (median %.3f ms: circuit,"
          " preprocess, verify_proof) minus `vk 32` (median %.3f ms: circuit, preprocess), %d alternating pairs.  Both walls are mostly process start,"
          " so read the difference with its quartiles; verify_proof's gate count only enters through log2 n squarings."
          % (d, d_lo, d_hi, v, k, args.reference_runs))


if __name__ == "__main__":
    main()
