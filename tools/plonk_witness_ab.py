#!/usr/bin/env python3
"""One-box A/B of the witness forms of the batch entry (bbgpu_plonk_construct_proof_batch_from) against expanded host wires, on this tree's library and
on the PARENT commit's.

    python tools/plonk_batch_ab.py --build-parent HEAD~1     # once, where the history is: the parent's sources -> barretenberg_amd/_variants/parent/
    python tools/plonk_witness_ab.py > profiles/plonk_witness_ab.txt

In one command on one box it alternates, --rounds times each, four child processes that each walk every (gates, count) cell:
  P   the parent commit's library: construct_proofs() with expanded wires in host memory
  W   this tree's library: the same call
  H   this tree's library: construct_proofs_from() with the composer's variables in host memory (one upload per lane, the expansion on the GPU)
  D   this tree's library: construct_proofs_from() with the variables in device memory (torch tensors, made before the timer starts: a witness that
      was produced on the GPU; nothing crosses the link)
Host clock around the calls (all end in a device synchronise); the uploads of P, W and H are inside the timer, the per-witness preprocess() a wires
caller pays is NOT (its saving is the caller's).  Each child warms up per size until the post-idle clock ramp is behind it and reports the median of
its repetitions per cell; the table gives the median of the rounds' medians in ms PER PROOF and the spread (max - min of the rounds' medians).  All
four sides must return equal bytes."""
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
PARENT_LIB = os.path.join(ROOT, "barretenberg_amd", "_variants", "parent", "barretenberg_amd", "libbbgpu.so")
WIRES = ("w_l", "w_r", "w_o")


def _witness(args):
    from barretenberg_amd.plonk import bench_circuit
    gates, j = args
    composer = bench_circuit(gates, A0 + j, B0 + 3 * j)
    *index, variables = composer.wire_map()
    return gates, j, composer.preprocess() if j == 0 else None, index, variables


def make_inputs(path, gates_list, max_count):
    """per size: the circuit state and the wire map once, the variables of max_count witnesses (the wires are variables[index])"""
    out = {}
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        for gates, j, st, index, variables in ex.map(_witness, [(g, j) for g in gates_list for j in range(max_count)]):
            if j == 0:
                for k, v in st.items():
                    out["%d/state/%s" % (gates, k)] = np.asarray(v)
                for k, a in zip(WIRES, index):
                    out["%d/index/%s" % (gates, k)] = a
            out["%d/v%d" % (gates, j)] = variables
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
        index = [z["%d/index/%s" % (gates, k)] for k in WIRES]
        vs = [z["%d/v%d" % (gates, j)] for j in range(max(counts))]
        srs = G.srs_generate(to_montgomery_limbs([SECRET % FR_MODULUS])[0], state["n"])
        P = Prover(G, state, srs)
        if mode == "wires":
            items = [tuple(np.ascontiguousarray(v[i]) for i in index) for v in vs]
            run = lambda count: P.construct_proofs(items[:count])  # noqa: E731
        else:
            P.set_wire_map(*index, len(vs[0]))
            if mode == "device":
                import torch
                items = [torch.from_numpy(v.view(np.int64)).cuda() for v in vs]
                torch.cuda.synchronize()
            else:
                items = vs
            run = lambda count: P.construct_proofs_from(items[:count])  # noqa: E731
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
            res["%d,%d" % (gates, count)] = {"ms": float(np.median(ts)), "sha": hashlib.sha256(proofs.tobytes()).hexdigest(),
                                             "n": state["n"], "num_variables": int(len(vs[0]))}
        P.destroy()
        G.srs_release(srs)
    G.shutdown()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--gates", type=int, nargs="+", default=[1 << 12, 1 << 14, 1 << 16, 1 << 18])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 8, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", choices=["wires", "host", "device"])
    ap.add_argument("--inputs")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.inputs, args.gates, args.counts, args.reps)
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s: run tools/plonk_batch_ab.py --build-parent REV where the history is" % args.parent_lib)
    sides = (("P", "wires", args.parent_lib), ("W", "wires", None), ("H", "host", None), ("D", "device", None))
    with tempfile.TemporaryDirectory() as tmp:
        inputs = os.path.join(tmp, "inputs.npz")
        t0 = time.perf_counter()
        make_inputs(inputs, args.gates, max(args.counts))
        print("# inputs: %d sizes x %d witnesses in %.1f s" % (len(args.gates), max(args.counts), time.perf_counter() - t0), flush=True)
        runs = {s[0]: [] for s in sides}
        for rnd in range(args.rounds):
            k = rnd % len(sides)
            for name, mode, libpath in sides[k:] + sides[:k]:  # the order rotates: no side always runs behind the same other one
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
                print("# round %d side %s done" % (rnd, name), file=sys.stderr, flush=True)  # progress, not part of the table
    print("# P = parent library, wires in host memory;  W = this library, the same call;  H = this library, variables in host memory;")
    print("# D = this library, variables in device memory (made before the timer starts)")
    print("# ms per proof: median of %d rounds' medians (spread = max - min of them); uploads are timed, per-witness preprocess() is not" % args.rounds)
    print("# the double-write variant of the expansion (G_WLAG and G_W at once, dropping the lanes' copy) was not tried: not in this table")
    print("%8s %5s | %18s | %18s | %18s | %18s | %5s %5s | bytes" % ("gates", "count", "P", "W", "H", "D", "W/H", "W/D"))
    stat, sizes = {}, {}
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
            sizes[g] = (runs["H"][0][key]["n"], runs["H"][0][key]["num_variables"])
            print("%8d %5d | %8.3f (%7.3f) | %8.3f (%7.3f) | %8.3f (%7.3f) | %8.3f (%7.3f) | %5.2f %5.2f | %s" % (
                g, c, row["P"][0], row["P"][1], row["W"][0], row["W"][1], row["H"][0], row["H"][1], row["D"][0], row["D"][1],
                row["W"][0] / row["H"][0], row["W"][0] / row["D"][0], "equal" if len(shas) == 1 else "DIFFERENT"))
    print("# all four sides return equal bytes in every cell: %s" % ("yes" if ok_bytes else "NO"))
    print("# bytes uploaded per lane: wires 3 n x 32, host variables num_variables x 32, device variables 0")
    for g, (n, nv) in sizes.items():
        print("#   %8d gates (n = %d, %d variables): wires %d, host variables %d (%.2f of the wires), device variables 0" % (
            g, n, nv, 3 * n * 32, nv * 32, nv / (3.0 * n)))

    def verdict(text, ok):
        print("# %s: %s" % (text, "holds" if ok else "FAILS"))
    worst = max(((abs(r["W"][0] - r["P"][0]) - max(r["P"][1], r["W"][1])), k) for k, r in stat.items())
    verdict("wires on this library are within the cell's spread of the parent's in every cell (worst excess %.3f ms at %s)" % worst, worst[0] <= 0)
    for name, label in (("H", "host variables"), ("D", "device variables")):
        worst = max(((r[name][0] - r["W"][0] - max(r["W"][1], r[name][1])), k) for k, r in stat.items())
        verdict("%s are not slower than wires on this library by more than the larger spread in every cell (worst excess %.3f ms at %s)" % (
            (label,) + worst), worst[0] <= 0)


if __name__ == "__main__":
    main()
