#!/usr/bin/env python3
"""One-box A/B of the opt-in witness check (bbgpu_plonk_set_witness_check) against the PARENT commit's library, and the cost of the check entries alone.

    python tools/plonk_batch_ab.py --build-parent HEAD~1     # once, where the history is: the parent's sources -> barretenberg_amd/_variants/parent/
    python tools/plonk_check_ab.py > profiles/plonk_check_ab.txt

In one command on one box it alternates, --rounds times each, three child processes that each walk every cell (gates, count; count 0 = the single entry,
set_witness outside the timer as a proving service keeps its witness resident; count > 0 = construct_proofs, uploads inside the timer):
  P    the parent commit's library (it has no flag)
  OFF  this tree's library, flag at its default 0
  ON   this tree's library, bbgpu_plonk_set_witness_check(prover, 1)
Host clock around the calls (all end in a device synchronise).  Each child warms up per cell until the post-idle clock ramp is behind it (DESIGN.md section
5) and reports the median of its repetitions; the table gives the median of the rounds' medians in ms PER PROOF and the spread (max - min of the rounds'
medians).  All three sides must return equal bytes.  The ON child also times bbgpu_plonk_check_witness / _check_witness_batch alone, and every child counts
how often one warm single proof and one warm batch of 8 at 2^14 gates pass the four funnels of bbgpu_fault_stats: P and OFF must agree."""
import argparse
import hashlib
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
import plonk_batch_ab as AB  # noqa: E402  (inputs, constants, the parent build)

CELLS = [(1 << 16, 0), (1 << 20, 0), (1 << 12, 8), (1 << 16, 8)]
FUNNEL_GATES = 1 << 14
FUNNELS = ("alloc_calls", "h2d_calls", "d2h_calls", "launch_checks")


def child(mode, inputs, cells, reps):
    from barretenberg_amd import BbGpu
    from barretenberg_amd.plonk import FR_MODULUS, Prover, to_montgomery_limbs
    z = np.load(inputs)
    G = BbGpu(0)
    res = {}
    for gates in sorted({g for g, _ in cells} | {FUNNEL_GATES}):
        state = {k.split("/", 2)[2]: z[k] for k in z.files if k.startswith("%d/state/" % gates)}
        state["n"] = int(state["n"])
        have = len([k for k in z.files if k.startswith("%d/w" % gates) and k.endswith("/w_l")])
        ws = [tuple(z["%d/w%d/%s" % (gates, j, k)] for k in ("w_l", "w_r", "w_o")) for j in range(have)]
        srs = G.srs_generate(to_montgomery_limbs([AB.SECRET % FR_MODULUS])[0], state["n"])
        P = Prover(G, state, srs)
        if mode == "on":
            P.set_witness_check(True)
        P.set_witness(*ws[0])

        def run(count):
            return P.construct_proofs(ws[:count]) if count else P.construct_proof()
        for g, count in cells + ([(FUNNEL_GATES, 0), (FUNNEL_GATES, 8)] if gates == FUNNEL_GATES else []):
            if g != gates:
                continue
            run(count)  # first use: circuit preparation, lanes, workspaces, the check's records
            if gates == FUNNEL_GATES:
                run(count)
                s0 = G.fault_stats()
                run(count)
                s1 = G.fault_stats()
                res["funnels,%d" % count] = {k: int(s1[k] - s0[k]) for k in FUNNELS}
                if (g, count) not in cells:
                    continue
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.2:  # past the post-idle clock ramp
                run(count)
            ts = []
            for _ in range(reps if gates < (1 << 18) else max(3, reps // 2)):
                t0 = time.perf_counter()
                proofs = run(count)
                ts.append((time.perf_counter() - t0) * 1e3 / max(count, 1))
            res["%d,%d" % (gates, count)] = {"ms": float(np.median(ts)), "sha": hashlib.sha256(np.asarray(proofs).tobytes()).hexdigest()}
            if mode == "on":  # the check entries alone
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    reports = P.check_witnesses(ws[:count]) if count else [P.check_witness()]
                    ts.append((time.perf_counter() - t0) * 1e3 / max(count, 1))
                assert all(r["gate_failures"] == 0 and r["copy_failures"] == 0 for r in reports)
                res["check,%d,%d" % (gates, count)] = {"ms": float(np.median(ts))}
        P.destroy()
        G.srs_release(srs)
    G.shutdown()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=AB.PARENT_LIB)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", choices=["parent", "off", "on"])
    ap.add_argument("--inputs")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.inputs, CELLS, args.reps)
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s: run tools/plonk_batch_ab.py --build-parent REV where the history is" % args.parent_lib)
    sides = (("P", "parent", args.parent_lib), ("OFF", "off", None), ("ON", "on", None))
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "inputs.npz")
        t0 = time.perf_counter()
        need = {}
        for g, c in CELLS + [(FUNNEL_GATES, 8)]:
            need[g] = max(need.get(g, 1), c)
        out = {}
        for g, c in sorted(need.items()):  # per size: the circuit state and as many witnesses of it as its largest cell takes
            sub = os.path.join(tmp, "in_%d.npz" % g)
            AB.make_inputs(sub, [g], c)
            with np.load(sub) as zz:
                out.update({k: zz[k] for k in zz.files})
        np.savez(inputs, **out)
        print("# inputs in %.1f s" % (time.perf_counter() - t0), flush=True)
        runs = {s[0]: [] for s in sides}
        for rnd in range(args.rounds):
            for name, mode, libpath in sides[rnd % 3:] + sides[:rnd % 3]:  # the order rotates: no side always runs behind the same other one
                env = dict(os.environ)
                env.pop("BBGPU_LIB", None)
                if libpath:
                    env["BBGPU_LIB"] = libpath
                cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--inputs", inputs, "--reps", str(args.reps)]
                r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.exit("child %s (round %d) failed: %s" % (name, rnd, r.stderr[-2000:]))
                runs[name].append(json.loads(line[0][7:]))
                print("# round %d side %s done" % (rnd, name), flush=True)
    print("# P = parent library;  OFF = this library, witness check off (the default);  ON = this library, witness check on")
    print("# count 0 = construct_proof (witness resident), count 8 = construct_proofs of 8 witnesses (uploads timed); ms per proof: median of %d rounds' "
          "medians (spread = max - min of them)" % args.rounds)
    print("%8s %5s | %18s | %18s | %18s | %8s | %8s | bytes" % ("gates", "count", "P", "OFF", "ON", "OFF/P", "ON/P"))
    stat = {}
    for g, c in CELLS:
        key = "%d,%d" % (g, c)
        row = {}
        for name in runs:
            ms = [r[key]["ms"] for r in runs[name]]
            row[name] = (float(np.median(ms)), max(ms) - min(ms))
        shas = {r[key]["sha"] for name in runs for r in runs[name]}
        stat[(g, c)] = row
        print("%8d %5d | %8.3f (%7.3f) | %8.3f (%7.3f) | %8.3f (%7.3f) | %8.4f | %8.4f | %s" % (
            g, c, row["P"][0], row["P"][1], row["OFF"][0], row["OFF"][1], row["ON"][0], row["ON"][1], row["OFF"][0] / row["P"][0],
            row["ON"][0] / row["P"][0], "equal" if len(shas) == 1 else "DIFFERENT"))
    print("# the check entries alone (ON child; count 8: bbgpu_plonk_check_witness_batch with its 8 uploads), ms per witness")
    for g, c in CELLS:
        ms = [r["check,%d,%d" % (g, c)]["ms"] for r in runs["ON"]]
        print("%8d %5d | %8.3f (%7.3f)" % (g, c, float(np.median(ms)), max(ms) - min(ms)))
    print("# funnel passes of one warm call at %d gates (alloc, h2d, d2h, launch checks)" % FUNNEL_GATES)
    fun = {}
    for name in runs:
        for c in (0, 8):
            vals = {json.dumps(r["funnels,%d" % c], sort_keys=True) for r in runs[name]}
            fun[(name, c)] = vals
            print("%4s count %d: %s" % (name, c, " / ".join(sorted(vals))))

    def verdict(text, ok):
        print("# %s: %s" % (text, "holds" if ok else "FAILS"))
    verdict("flag off passes every funnel as often as the parent", all(fun[("P", c)] == fun[("OFF", c)] and len(fun[("P", c)]) == 1 for c in (0, 8)))
    worst = max(((abs(r["OFF"][0] - r["P"][0]) - max(r["P"][1], r["OFF"][1])), k) for k, r in stat.items())
    verdict("flag off is within the spread of the parent in every cell (worst excess %.3f ms at %s)" % worst, worst[0] <= 0)
    r = stat[(1 << 16, 8)]
    verdict("2^16 gates, batch of 8: the check costs %.2f %% of the parent's per-proof time (bar for a closer look: 5 %%)" % (100 * (r["ON"][0] / r["P"][0] - 1)),
            r["ON"][0] <= 1.05 * r["P"][0])


if __name__ == "__main__":
    main()
