#!/usr/bin/env python3
"""One-box A/B of bbgpu_plonk_construct_proof_batch against the single-proof path of the PARENT commit's library.

    python tools/plonk_batch_ab.py --build-parent HEAD~1     # once, where the history is: the parent's sources -> barretenberg_amd/_variants/parent/
    python tools/plonk_batch_ab.py > profiles/plonk_batch_ab.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/plonk_batch_ab.py --once 65536 8   # -> profiles/plonk_batch_kernel_stats.csv

In one command on one box it alternates, --rounds times each, three child processes that each walk every (gates, count) cell:
  A   the parent commit's library: count x (set_witness + construct_proof)
  B   this tree's library: construct_proofs() with the same witnesses
  A'  this tree's library: the loop of A (the single path must not have moved)
Host clock around the calls (all end in a device synchronise; the witness uploads are inside the timer on every side).  Each child warms up per size
until the post-idle clock ramp is behind it (about 120 ms of work) and reports the median of its repetitions per cell; the table
gives the median of the rounds' medians in ms PER PROOF and the spread (max - min of the rounds' medians).  Boxes differ by +-5 % on one binary, which is
why the sides alternate on one box and the margin of the verdict lines is this run's own spread.  A and B must return equal bytes."""
import argparse
import concurrent.futures
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

A0 = 0x0777777788888888555555556666666633333333444444441111111122222222
B0 = 0x0ABCDEFABCDEFABC1234123412341234DDDDEEEEFFFF00009999AAAABBBBCCCC
SECRET = 0x0123456789ABCDEF0F1E2D3C4B5A6978FEDCBA98765432100123456789ABCDEF
PARENT_DIR = os.path.join(ROOT, "barretenberg_amd", "_variants", "parent")
PARENT_LIB = os.path.join(PARENT_DIR, "barretenberg_amd", "libbbgpu.so")


def build_parent(rev):
    """the library of commit `rev`, from its own sources, in a directory of its own"""
    os.makedirs(PARENT_DIR, exist_ok=True)
    ar = subprocess.run(["git", "archive", rev, "barretenberg_amd/csrc", "include"], cwd=ROOT, check=True, capture_output=True)
    subprocess.run(["tar", "-x", "-C", PARENT_DIR], input=ar.stdout, check=True)
    subprocess.run(["make", "-C", os.path.join(PARENT_DIR, "barretenberg_amd", "csrc"), "-j8"], check=True, stdout=subprocess.DEVNULL)
    print("built", PARENT_LIB)


def _witness(args):
    from barretenberg_amd.plonk import bench_circuit
    gates, j = args
    st = bench_circuit(gates, A0 + j, B0 + 3 * j).preprocess()
    return gates, j, st if j == 0 else {k: st[k] for k in ("w_l", "w_r", "w_o")}


def make_inputs(path, gates_list, max_count):
    """circuit state per size and max_count witnesses of it, written once for all children (the composer mirror is Python: 4 s per 2^18 gates)"""
    out = {}
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        for gates, j, st in ex.map(_witness, [(g, j) for g in gates_list for j in range(max_count)]):
            if j == 0:
                for k, v in st.items():
                    out["%d/state/%s" % (gates, k)] = np.asarray(v)
            for k in ("w_l", "w_r", "w_o"):
                out["%d/w%d/%s" % (gates, j, k)] = st[k]
    np.savez(path, **out)


def child(mode, inputs, gates_list, counts, reps):
    from barretenberg_amd import BbGpu
    from barretenberg_amd.plonk import FR_MODULUS, Prover, to_montgomery_limbs
    z = np.load(inputs)
    G = BbGpu(0)
    res = {}
    for gates in gates_list:
        state = {k.split("/", 2)[2]: z[k] for k in z.files if k.startswith("%d/state/" % gates)}
        state["n"] = int(state["n"])
        ws = [tuple(z["%d/w%d/%s" % (gates, j, k)] for k in ("w_l", "w_r", "w_o")) for j in range(max(counts))]
        srs = G.srs_generate(to_montgomery_limbs([SECRET % FR_MODULUS])[0], state["n"])
        P = Prover(G, state, srs)

        def run(count):
            if mode == "batch":
                return P.construct_proofs(ws[:count])
            out = np.zeros((count, 120), dtype=np.uint64)
            for j in range(count):
                P.set_witness(*ws[j])
                out[j] = P.construct_proof()
            return out
        run(max(counts))  # first use: circuit preparation, lanes, workspaces
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:  # past the post-idle clock ramp
            run(1)
        for count in counts:
            run(count)
            ts = []
            for _ in range(reps if gates < (1 << 18) else max(3, reps // 2)):
                t0 = time.perf_counter()
                proofs = run(count)
                ts.append((time.perf_counter() - t0) * 1e3 / count)
            res["%d,%d" % (gates, count)] = {"ms": float(np.median(ts)), "sha": hashlib.sha256(proofs.tobytes()).hexdigest()}
        P.destroy()
        G.srs_release(srs)
    G.shutdown()
    print("RESULT " + json.dumps(res))


def once(gates, count):
    from barretenberg_amd import BbGpu
    from barretenberg_amd.plonk import FR_MODULUS, Prover, to_montgomery_limbs
    ws = [_witness((gates, j))[2] for j in range(count)]
    G = BbGpu(0)
    srs = G.srs_generate(to_montgomery_limbs([SECRET % FR_MODULUS])[0], ws[0]["n"])
    P = Prover(G, ws[0], srs)
    P.construct_proofs([(w["w_l"], w["w_r"], w["w_o"]) for w in ws])
    print("one batch of %d at %d gates: %s" % (count, gates, P.batch_timing()))
    P.destroy()
    G.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-parent", metavar="REV")
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--gates", type=int, nargs="+", default=[1 << 12, 1 << 14, 1 << 16, 1 << 18])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", choices=["loop", "batch"])
    ap.add_argument("--inputs")
    ap.add_argument("--once", type=int, nargs=2, metavar=("GATES", "COUNT"), help="one batch and nothing else: the workload of a rocprofv3 --kernel-trace --stats run")
    args = ap.parse_args()
    if args.once:
        return once(*args.once)
    if args.build_parent:
        return build_parent(args.build_parent)
    if args.child:
        return child(args.child, args.inputs, args.gates, args.counts, args.reps)
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s: run --build-parent REV where the history is" % args.parent_lib)
    sides = (("A", "loop", args.parent_lib), ("B", "batch", None), ("A'", "loop", None))
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "inputs.npz")
        t0 = time.perf_counter()
        make_inputs(inputs, args.gates, max(args.counts))
        print("# inputs: %d sizes x %d witnesses in %.1f s" % (len(args.gates), max(args.counts), time.perf_counter() - t0), flush=True)
        runs = {s[0]: [] for s in sides}
        for rnd in range(args.rounds):
            for name, mode, libpath in sides[rnd % 3:] + sides[:rnd % 3]:  # the order rotates: no side always runs behind the same other one
                env = dict(os.environ)
                env.pop("BBGPU_LIB", None)
                if libpath:
                    env["BBGPU_LIB"] = libpath
                cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--inputs", inputs, "--reps", str(args.reps), "--gates"] + \
                    [str(g) for g in args.gates] + ["--counts"] + [str(c) for c in args.counts]
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.exit("child %s (round %d) failed: %s" % (name, rnd, r.stderr[-2000:]))
                runs[name].append(json.loads(line[0][7:]))
                print("# round %d side %s done" % (rnd, name), flush=True)
    print("# A = parent library, count x (set_witness + construct_proof);  B = construct_proofs;  A' = the loop of A on this library")
    print("# ms per proof: median of %d rounds' medians (spread = max - min of them)" % args.rounds)
    print("%8s %5s | %18s | %18s | %18s | %6s | bytes" % ("gates", "count", "A", "B", "A'", "A/B"))
    stat = {}
    ok_bytes = True
    for g in args.gates:
        for c in args.counts:
            key = "%d,%d" % (g, c)
            row = {}
            for name in runs:
                ms = [r[key]["ms"] for r in runs[name]]
                row[name] = (float(np.median(ms)), max(ms) - min(ms))
            shas = {r[key]["sha"] for name in runs for r in runs[name]}
            ok_bytes = ok_bytes and len(shas) == 1
            stat[(g, c)] = row
            print("%8d %5d | %8.3f (%7.3f) | %8.3f (%7.3f) | %8.3f (%7.3f) | %6.2f | %s" % (
                g, c, row["A"][0], row["A"][1], row["B"][0], row["B"][1], row["A'"][0], row["A'"][1], row["A"][0] / row["B"][0],
                "equal" if len(shas) == 1 else "DIFFERENT"))
    print("# A and B return equal bytes in every cell: %s" % ("yes" if ok_bytes else "NO"))

    def verdict(text, ok):
        print("# %s: %s" % (text, "holds" if ok else "FAILS"))
    if (1 << 16, 8) in stat:
        r = stat[(1 << 16, 8)]
        m = max(r["A"][1], r["B"][1])
        verdict("2^16 gates, count 8: B %.3f < A %.3f - %.3f (the larger spread)" % (r["B"][0], r["A"][0], m), r["B"][0] < r["A"][0] - m)
    for g in args.gates:
        if (g, 1) in stat:
            r = stat[(g, 1)]
            m = max(r["A"][1], r["B"][1])
            verdict("%d gates, count 1: B %.3f <= A %.3f + %.3f" % (g, r["B"][0], r["A"][0], m), r["B"][0] <= r["A"][0] + m)
    worst = max(((abs(r["A'"][0] - r["A"][0]) - max(r["A"][1], r["A'"][1])), k) for k, r in stat.items())
    verdict("the single path on this library is within the spread of the parent's in every cell (worst excess %.3f ms at %s)" % worst, worst[0] <= 0)


if __name__ == "__main__":
    main()
