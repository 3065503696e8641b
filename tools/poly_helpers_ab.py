#!/usr/bin/env python3
"""One-box A/B of the single-vector polynomial helpers (csrc/poly.hip through the C ABI) between the PARENT commit's library and this tree's.

    make -C barretenberg_amd/csrc variant NAME=parent        # in a checkout of the parent: -> barretenberg_amd/_variants/libbbgpu_parent.so
    python tools/poly_helpers_ab.py > profiles/poly_one_text_ab.txt

In one command on one box it alternates, --rounds times each and in rotating order, a child process on the parent's library (P) and one on this tree's
(N).  A child times product_scan_device, compute_kate_opening_coefficients_device, evaluate_device, batch_invert_device and
divide_by_pseudo_vanishing_polynomial_device at 2^16 and 2^20 elements: HIP events around every call on a stream of its own, the median of 20 calls
after 3 warm ones, and a hash of every output.  The table gives the median of the rounds' medians in ms and the spread (max - min of them); the bar of
a cell is N <= P + P's spread -- the noise of that box, a refactor gets no other allowance -- and the bytes must be equal."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

PARENT_LIB = os.path.join(ROOT, "barretenberg_amd", "_variants", "libbbgpu_parent.so")
SIZES = (1 << 16, 1 << 20)
HELPERS = ("product_scan", "kate_opening", "evaluate", "batch_invert", "divide_vanishing")


def child(warm, calls):
    import torch
    from barretenberg_amd import BbGpu
    from oracle.pyoracle import Oracle
    O, G = Oracle(), BbGpu(device=0)
    s = torch.cuda.Stream()
    out = {}
    for n in SIZES:
        v = O.random_scalars(0xAB + n, n)
        z = O.random_scalars(0xAC + n, 1)[0]
        src = torch.from_numpy(v.view(np.int64)).cuda()
        dst = torch.zeros_like(src)
        work = src.clone()

        def restore():
            work.copy_(src)  # on torch's stream; the synchronise below orders it before the timed call

        runs = {
            "product_scan": (lambda: G.product_scan_device(src.data_ptr(), dst.data_ptr(), n, False, False, stream=s.cuda_stream), lambda: dst, None),
            "kate_opening": (lambda: G.compute_kate_opening_coefficients_device(src.data_ptr(), dst.data_ptr(), n, z, stream=s.cuda_stream), lambda: dst, None),
            "evaluate": (lambda: G.evaluate_device(src.data_ptr(), n, z, stream=s.cuda_stream), None, None),
            "batch_invert": (lambda: G.batch_invert_device(work.data_ptr(), n, stream=s.cuda_stream), lambda: work, restore),  # in place
            "divide_vanishing": (lambda: G.divide_by_pseudo_vanishing_polynomial_device(work.data_ptr(), n // 4, n, stream=s.cuda_stream), lambda: work, restore),
        }
        for name in HELPERS:
            call, result, before = runs[name]
            ms, ret = [], None
            for k in range(warm + calls):
                if before:
                    before()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                ret = call()
                e1.record(s)
                torch.cuda.synchronize()
                if k >= warm:
                    ms.append(e0.elapsed_time(e1))
            h = hashlib.sha256()
            if ret is not None:
                h.update(np.ascontiguousarray(ret).tobytes())
            if result:
                h.update(result().cpu().numpy().tobytes())
            out["%s,%d" % (name, n)] = {"ms": float(np.median(ms)), "sha": h.hexdigest()[:16]}
    G.shutdown()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.warm, args.calls)
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s: make -C barretenberg_amd/csrc variant NAME=parent in a checkout of the parent" % args.parent_lib)
    sides = (("P", args.parent_lib), ("N", None))
    runs = {s[0]: [] for s in sides}
    for rnd in range(args.rounds):
        for name, libpath in sides[rnd % 2:] + sides[:rnd % 2]:  # the order rotates
            env = dict(os.environ)
            env.pop("BBGPU_LIB", None)
            if libpath:
                env["BBGPU_LIB"] = libpath
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--warm", str(args.warm), "--calls", str(args.calls)]
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit("child %s (round %d) failed with %d: %s" % (name, rnd, r.returncode, r.stderr[-2000:]))
            runs[name].append(json.loads(line[0][7:]))
            print("# round %d side %s done" % (rnd, name), flush=True)
    print("# P = parent library;  N = this library.  ms per call by HIP events: median of %d rounds' medians of %d calls (spread = max - min of them)"
          % (args.rounds, args.calls))
    print("%-18s %8s | %18s | %18s | %7s | %s | bytes" % ("helper", "n", "P", "N", "N/P", "N <= P + P's spread"))
    all_ok = True
    for name in HELPERS:
        for n in SIZES:
            key = "%s,%d" % (name, n)
            row = {}
            for side in runs:
                ms = [r[key]["ms"] for r in runs[side]]
                row[side] = (float(np.median(ms)), max(ms) - min(ms))
            equal = len({r[key]["sha"] for side in runs for r in runs[side]}) == 1
            ok = row["N"][0] <= row["P"][0] + row["P"][1]
            all_ok = all_ok and ok and equal
            print("%-18s %8d | %8.4f (%7.4f) | %8.4f (%7.4f) | %7.4f | %19s | %s" % (name, n, row["P"][0], row["P"][1], row["N"][0], row["N"][1], row["N"][0] / row["P"][0],
                                                                                   "holds" if ok else "FAILS", "equal" if equal else "DIFFERENT"))
    print("# every cell within the bar, equal bytes in every cell: %s" % ("holds" if all_ok else "FAILS"))
    print("# the rounds' medians, in the order run")
    for name in HELPERS:
        for n in SIZES:
            key = "%s,%d" % (name, n)
            print("# %-18s %8d | %s" % (name, n, " | ".join("%s %s" % (side, " ".join("%.4f" % r[key]["ms"] for r in runs[side])) for side in runs)))


if __name__ == "__main__":
    main()
