"""What bbgpu_plonk_verify_multi costs against one bbgpu_plonk_verify_batch per circuit (profiles/plonk_verify_multi.txt is this tool's output): one
process on one MI355X, both libraries loaded side by side -- the in-tree build (child) and the PARENT commit's build (--parent-lib) -- every leg warm,
the two legs of a cell alternating inside every pair (the order swapped from pair to pair).  Wall milliseconds per CALL around the C entries, Python
binding included; every call ends synchronised (it returns the verdict).  Proofs: the honest proofs of tests/golden/plonk_verify.json's circuits,
repeated to the count; fixed seed, no LOCATE; every report is checked to be good.
  1. G = 1, 2, 4, 6 circuits at 256 and at 16 proofs per circuit, the queue's labels round-robin: ONE mixed call (child) against G calls of
     bbgpu_plonk_verify_batch (parent), the proofs already split by circuit outside the timed window.  "gain" is printed only where EVERY mixed time
     of the cell's pairs lies below its pair's sum of separate calls.
  2. bbgpu_plonk_verify_batch, parent against child, at 256 and 2^14 proofs of one circuit.  "no regression" is printed only where the child's median
     lies within the parent's median plus the spread (the parent's interquartile range in this run).
  3. G = 1 through bbgpu_plonk_verify_multi against bbgpu_plonk_verify_batch (both child), at 256 and 2^14 proofs: one call since both entries run
     one driver, which takes the single-circuit kernels whenever the call names one verifier.
  4. bbgpu_plonk_verify_multi, parent against child (a parent that has the entry), G = 1, 2, 4, 6 at 256 proofs per circuit and G = 1 at 2^14: section
     2's rule.
--sections picks some of the four, e.g. to repeat a cell with more pairs.
Usage: make the parent's library once (barretenberg_amd/csrc: `make variant NAME=parent` in a checkout of the parent, copied to
barretenberg_amd/_variants/libbbgpu_parent.so), then  python tools/plonk_verify_multi_bench.py [--pairs 31] [--parent-lib PATH]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARENT_LIB = os.path.join(ROOT, "barretenberg_amd", "_variants", "libbbgpu_parent.so")
SEED = np.arange(1, 5, dtype=np.uint64)


def stats(ts):
    q = statistics.quantiles(ts, n=4)
    return dict(med=statistics.median(ts), lo=min(ts), hi=max(ts), iqr=q[2] - q[0])


def show(name, ts):
    s = stats(ts)
    return "%s %7.3f (min %7.3f max %7.3f iqr %6.3f)" % (name, s["med"], s["lo"], s["hi"], s["iqr"])


def timed(call):
    t0 = time.perf_counter()
    rep = call()
    t1 = time.perf_counter()
    assert rep is True or rep.ok, rep.as_dict()
    return (t1 - t0) * 1e3


def pairs(n, leg_a, leg_b):
    """n alternating pairs after one warm pair; the order inside a pair swaps from pair to pair -> the two lists of times, pair by pair"""
    a, b = [], []
    for k in range(n + 1):
        if k % 2:
            tb, ta = timed(leg_b), timed(leg_a)
        else:
            ta, tb = timed(leg_a), timed(leg_b)
        if k:
            a.append(ta)
            b.append(tb)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=31)
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--sections", default="1,2,3,4")
    args = ap.parse_args()
    from barretenberg_amd import BbGpu
    from tests.plonk_verify_cases import fixture
    from tests.plonk_verify_multi_cases import CIRCUITS, honest_batch, index
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s (see the usage)" % args.parent_lib)
    child = BbGpu(device=0)
    os.environ["BBGPU_LIB"] = args.parent_lib
    parent = BbGpu(device=0)
    del os.environ["BBGPU_LIB"]
    sections = {int(x) for x in args.sections.split(",")}
    g2_x, circuits, _ = fixture()
    hc = [child.plonk_verifier_create(circuits[c]["n"], circuits[c]["widgets"], circuits[c]["vk"], g2_x) for c in CIRCUITS]
    hp = [parent.plonk_verifier_create(circuits[c]["n"], circuits[c]["widgets"], circuits[c]["vk"], g2_x) for c in CIRCUITS]
    print("# child %s, parent %s; wall ms per CALL: median (min, max, interquartile range) of %d alternating pairs after a warm pair"
          % (child.version(), parent.version(), args.pairs))

    print("\n1. one mixed call (child) against G calls of bbgpu_plonk_verify_batch (parent); circuits: the first G of %s" % ", ".join(CIRCUITS))
    for per in (256, 16) if 1 in sections else ():
        for G in (1, 2, 4, 6):
            labels = (np.arange(G * per) % G).astype(np.uint32)
            proofs = honest_batch(labels)
            split = [np.ascontiguousarray(proofs[labels == c]) for c in range(G)]

            def separate():
                return all(parent.plonk_verify_batch(hp[c], split[c], SEED).ok for c in range(G))
            mixed, sep = pairs(args.pairs, lambda: child.plonk_verify_multi(hc[:G], labels, proofs, SEED), separate)
            below = sum(m < s for m, s in zip(mixed, sep))
            saved = statistics.median(s - m for m, s in zip(mixed, sep))
            verdict = "gain: every mixed time below its pair's separate calls" if below == len(mixed) else "no gain stated: %d of %d pairs below" % (below, len(mixed))
            print("G %d x %3d proofs  %s  %s  paired difference median %+7.3f  %s"
                  % (G, per, show("mixed", mixed), show("separate", sep), saved, verdict), flush=True)

    one = np.zeros(1 << 14, dtype=np.uint32) + index("standard/32")
    big = honest_batch(one)

    def regression_line(what, tp, tc):
        sp, sc = stats(tp), stats(tc)
        holds = sc["med"] <= sp["med"] + sp["iqr"]
        print("%s  %s  %s  %s" % (what, show("parent", tp), show("child", tc),
                                  "no regression: the child's median within the parent's plus its spread" if holds else
                                  "REGRESSION by this run's rule: the child's median is above the parent's plus its spread"), flush=True)

    print("\n2. bbgpu_plonk_verify_batch, parent against child (standard/32)")
    for count in (256, 1 << 14) if 2 in sections else ():
        pr = np.ascontiguousarray(big[:count])
        tp, tc = pairs(args.pairs, lambda: parent.plonk_verify_batch(hp[0], pr, SEED), lambda: child.plonk_verify_batch(hc[0], pr, SEED))
        regression_line("count %5d" % count, tp, tc)

    print("\n3. G = 1 through bbgpu_plonk_verify_multi against bbgpu_plonk_verify_batch, both child (standard/32)")
    for count in (256, 1 << 14) if 3 in sections else ():
        pr, lb = np.ascontiguousarray(big[:count]), np.zeros(count, dtype=np.uint32)
        split_m, split_b = [], []

        def multi():
            rep = child.plonk_verify_multi(hc[:1], lb, pr, SEED)
            split_m.append(child.plonk_verify_last_timing())
            return rep

        def batch():
            rep = child.plonk_verify_batch(hc[0], pr, SEED)
            split_b.append(child.plonk_verify_last_timing())
            return rep
        tm, tb = pairs(args.pairs, multi, batch)
        sm, sb = stats(tm), stats(tb)
        terms = [statistics.median(s["terms_ms"] for s in sp[1:]) for sp in (split_m, split_b)]
        note = "slower by more than the spread" if sm["med"] > sb["med"] + sb["iqr"] else "within the spread" if sm["med"] >= sb["med"] - sb["iqr"] else "faster by more than the spread"
        print("count %5d  %s  %s  upload + k_verify_terms + read-back: multi %6.3f batch %6.3f  multi is %s"
              % (count, show("multi", tm), show("batch", tb), terms[0], terms[1], note), flush=True)

    print("\n4. bbgpu_plonk_verify_multi, parent against child; circuits as in 1, the labels round-robin")
    if 4 in sections and not hasattr(parent.lib, "bbgpu_plonk_verify_multi"):
        print("skipped: the parent has no such entry")
    elif 4 in sections:
        for G, per in ((1, 256), (2, 256), (4, 256), (6, 256), (1, 1 << 14)):
            labels = (np.arange(G * per) % G).astype(np.uint32)
            proofs = honest_batch(labels)
            tp, tc = pairs(args.pairs, lambda: parent.plonk_verify_multi(hp[:G], labels, proofs, SEED), lambda: child.plonk_verify_multi(hc[:G], labels, proofs, SEED))
            regression_line("G %d x %5d proofs" % (G, per), tp, tc)
    for g, hs in ((child, hc), (parent, hp)):
        for h in hs:
            g.plonk_verifier_destroy(h)
        g.shutdown()


if __name__ == "__main__":
    main()
