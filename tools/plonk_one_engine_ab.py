#!/usr/bin/env python3
"""One-box A/B of the one-engine prover (single proofs run through the lane engine) against the PARENT commit's library, which still had a single-proof
path of its own.

    python tools/plonk_batch_ab.py --build-parent HEAD~1     # once, where the history is: the parent's sources -> barretenberg_amd/_variants/parent/
    python tools/plonk_one_engine_ab.py > profiles/plonk_one_engine_ab.txt

In one command on one box it alternates, --rounds times each and in rotating order, a child on the parent's library (P) and a child on this tree's (N).  Both
walk the cells of tools/plonk_check_ab.py's child (count 0 = construct_proof with the witness resident, count 8 = construct_proofs of 8 witnesses, uploads
timed) and count the funnel passes of one warm single proof and one warm batch of 8 at 2^14 gates.  The table gives the median of the rounds' medians in ms
PER PROOF and the spread (max - min of the rounds' medians); the bar of every cell is N <= P + the larger spread, and the bytes must be equal."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import plonk_batch_ab as AB  # noqa: E402  (inputs, the parent build)
import plonk_check_ab as CK  # noqa: E402  (the child)

CELLS = [(1 << 12, 0), (1 << 16, 0), (1 << 20, 0), (1 << 21, 0), (1 << 12, 8), (1 << 16, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=AB.PARENT_LIB)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--inputs")
    args = ap.parse_args()
    if args.child:
        return CK.child("off", args.inputs, CELLS, args.reps)
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s: run tools/plonk_batch_ab.py --build-parent REV where the history is" % args.parent_lib)
    sides = (("P", args.parent_lib), ("N", None))
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "inputs.npz")
        t0 = time.perf_counter()
        need = {}
        for g, c in CELLS + [(CK.FUNNEL_GATES, 8)]:
            need[g] = max(need.get(g, 1), c)
        out = {}
        for g, c in sorted(need.items()):  # per size: the circuit state and as many witnesses of it as its largest cell takes
            sub = os.path.join(tmp, "in_%d.npz" % g)
            AB.make_inputs(sub, [g], c)
            with np.load(sub) as zz:
                out.update({k: zz[k] for k in zz.files})
            os.remove(sub)
        np.savez(inputs, **out)
        del out
        print("# inputs in %.1f s" % (time.perf_counter() - t0), flush=True)
        runs = {s[0]: [] for s in sides}
        for rnd in range(args.rounds):
            for name, libpath in sides[rnd % 2:] + sides[:rnd % 2]:  # the order rotates
                env = dict(os.environ)
                env.pop("BBGPU_LIB", None)
                if libpath:
                    env["BBGPU_LIB"] = libpath
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--inputs", inputs, "--reps", str(args.reps)]
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.exit("child %s (round %d) failed: %s" % (name, rnd, r.stderr[-2000:]))
                runs[name].append(json.loads(line[0][7:]))
                print("# round %d side %s done" % (rnd, name), flush=True)
    print("# P = parent library (a single-proof path of its own);  N = this library (single proofs through the lane engine)")
    print("# count 0 = construct_proof (witness resident), count 8 = construct_proofs of 8 witnesses (uploads timed); ms per proof: median of %d rounds' "
          "medians (spread = max - min of them)" % args.rounds)
    print("%8s %5s | %18s | %18s | %8s | %s | bytes" % ("gates", "count", "P", "N", "N/P", "N <= P + spread"))
    all_ok = True
    for g, c in CELLS:
        key = "%d,%d" % (g, c)
        row = {}
        for name in runs:
            ms = [r[key]["ms"] for r in runs[name]]
            row[name] = (float(np.median(ms)), max(ms) - min(ms))
        equal = len({r[key]["sha"] for name in runs for r in runs[name]}) == 1
        ok = row["N"][0] <= row["P"][0] + max(row["P"][1], row["N"][1])
        all_ok = all_ok and ok and equal
        print("%8d %5d | %8.3f (%7.3f) | %8.3f (%7.3f) | %8.4f | %15s | %s" % (g, c, row["P"][0], row["P"][1], row["N"][0], row["N"][1], row["N"][0] / row["P"][0],
                                                                          "holds" if ok else "FAILS", "equal" if equal else "DIFFERENT"))
    print("# funnel passes of one warm call at %d gates (alloc, h2d, d2h, launch checks)" % CK.FUNNEL_GATES)
    for name in runs:
        for c in (0, 8):
            print("%4s count %d: %s" % (name, c, " / ".join(sorted({json.dumps(r["funnels,%d" % c], sort_keys=True) for r in runs[name]}))))
    print("# every cell within the bar, equal bytes in every cell: %s" % ("holds" if all_ok else "FAILS"))


if __name__ == "__main__":
    main()
