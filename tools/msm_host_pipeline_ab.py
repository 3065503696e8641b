#!/usr/bin/env python3
"""One-box A/B of the host-pointer MSM entries (bbgpu_msm_g1, bbgpu_msm_g1_batch) against the PARENT commit's library, for a change that must leave
their speed as it was (the slot pipeline of csrc/capi.hip).

    make -C barretenberg_amd/csrc variant NAME=parent        # in a checkout of the parent; copy ../_variants/libbbgpu_parent.so here
    python tools/msm_host_pipeline_ab.py > profiles/msm_host_pipeline_ab.txt

In one command on one box it alternates, --rounds times each and in rotating order, a child on the parent's library (P) and a child on this tree's (N).
A child takes wall-clock medians around the calls, pageable host buffers, the point table cached: pippenger at 2^20 (tools/boundary_ab.py), the three-job
2^20 batch (bench.py's boundary.msm_g1_batch_3x2e20), pippenger at 100 / 4096 / 2^16 points (tools/small_sizes.py: ~0.35 ms calls, host overhead shows),
and both 2^20 calls in the EXACT cache mode (tools/validate_ab.py).  The table gives the median of the rounds' medians and the spread (max - min of them);
a cell passes when N lies within P's own spread of P, or below."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

PARENT_LIB = os.path.join(ROOT, "barretenberg_amd", "_variants", "libbbgpu_parent.so")
CELLS = ["msm_2e20", "batch3_2e20", "msm_100", "msm_4096", "msm_2e16", "msm_2e20_exact", "batch3_2e20_exact"]


def med(f, reps, warm):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def child():
    from barretenberg_amd import BbGpu
    G = BbGpu(0)
    rng = np.random.default_rng(7)
    x = rng.integers(0, 1 << 64, size=4, dtype=np.uint64)
    x[3] &= np.uint64(0x1FFFFFFFFFFFFFFF)
    n = 1 << 20
    h0, table = G.srs_generate(x, n, True)
    G.srs_release(h0)  # the host-pointer calls register the table on first sight
    hs = []
    for k in range(3):
        sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)
        hs.append(sc)
    turn = [0]
    digest = hashlib.sha256()

    def one(m=n, tab=table):
        turn[0] += 1
        return G.pippenger(hs[turn[0] % 3][:m], tab, m)

    def batch():
        return G.batched_scalar_multiplications([(table, h, n) for h in hs])
    out = {}
    out["msm_2e20"] = med(one, 10, 3)
    out["batch3_2e20"] = med(batch, 10, 3)
    for name, m in (("msm_100", 100), ("msm_4096", 4096), ("msm_2e16", 1 << 16)):
        tab = np.ascontiguousarray(table[:2 * m]).copy()  # a table of its own: m = 100 is uploaded per call, the others are cached on first sight
        out[name] = med(lambda: one(m, tab), 31, 3)
        turn[0] = 0
        digest.update(one(m, tab).tobytes())
    h = G.srs_register(table)
    G.srs_set_validate(h, 1)
    out["msm_2e20_exact"] = med(one, 10, 3)
    out["batch3_2e20_exact"] = med(batch, 5, 2)
    G.srs_set_validate(h, 0)
    turn[0] = 0
    digest.update(one().tobytes())
    for o in batch():
        digest.update(o.tobytes())
    out["digest"] = digest.hexdigest()[:16]
    G.shutdown()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s (see the head of this file)" % args.parent_lib)
    sides = (("P", args.parent_lib), ("N", None))
    runs = {s[0]: [] for s in sides}
    for rnd in range(args.rounds):
        for name, libpath in sides[rnd % 2:] + sides[:rnd % 2]:  # the order rotates
            env = dict(os.environ)
            env.pop("BBGPU_LIB", None)
            if libpath:
                env["BBGPU_LIB"] = libpath
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit("child %s (round %d) failed with %d: %s" % (name, rnd, r.returncode, r.stderr[-2000:]))
            runs[name].append(json.loads(line[0][7:]))
            print("# round %d side %s done" % (rnd, name), flush=True)
    print("# P = parent library;  N = this library.  Wall-clock ms per call: median of %d alternating rounds' medians (spread = max - min of them)" % args.rounds)
    print("%-18s | %-26s | %-26s | %6s | N <= P + P's spread" % ("call", "P", "N", "N/P"))
    all_ok, rounds = True, []
    for cell in CELLS:
        p = [r[cell] for r in runs["P"]]
        q = [r[cell] for r in runs["N"]]
        pm, qm, ps, qs = float(np.median(p)), float(np.median(q)), max(p) - min(p), max(q) - min(q)
        ok = qm <= pm + ps
        all_ok = all_ok and ok
        print("%-18s | %8.4f (spread %7.4f) | %8.4f (spread %7.4f) | %6.3f | %s" % (cell, pm, ps, qm, qs, qm / pm, "ok" if ok else "OUTSIDE"))
        rounds.append("# %-18s P %s | N %s" % (cell, " ".join("%.4f" % v for v in p), " ".join("%.4f" % v for v in q)))
    print("# the rounds' medians, in the order run:\n" + "\n".join(rounds))
    same = len({r["digest"] for side in runs.values() for r in side}) == 1
    print("# results identical across all runs: %s" % same)
    print("# summary: %s" % ("every call within the parent's spread" if all_ok and same else "SEE ABOVE"))
    return 0 if all_ok and same else 1


if __name__ == "__main__":
    sys.exit(main())
