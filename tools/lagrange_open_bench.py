"""What evaluation and opening in evaluation form cost against the transform path, and what bbgpu_srs_lagrange_check costs against its two MSMs
(profiles/lagrange_open.txt is this tool's output): one process on one MI355X, both libraries loaded side by side -- the in-tree build (child) and the
PARENT commit's build (--parent-lib), which runs the comparison side of (a) and (b) -- every leg warm, the two legs of a cell alternating inside every
pair (the order swapped from pair to pair).  Wall milliseconds per CALL SEQUENCE around the C entries, Python binding included, each leg ended by a device
synchronise.  n = 2^16 and 2^20, batch 1 and 8, random values, one random z (off the domain), the legacy default stream.
  (a) evaluation: bbgpu_fr_evaluate_lagrange_device (child) against bbgpu_ntt_device_batch(IFFT) + one bbgpu_fr_evaluate_device per polynomial (parent).
      The transform runs in place on a buffer of its own, again and again: its time does not depend on the data, and the copy a caller who wants to keep
      the values would need is NOT charged to it.
  (b) opening: bbgpu_kate_opening_lagrange_device (child) against IFFT + one bbgpu_kate_opening_device per polynomial (parent), f(z) returned by both;
      then each path followed by its commitments, one device MSM per polynomial -- over the Lagrange handle (child) and the monomial handle (parent;
      behind a device synchronise, since the coefficient-form entry returns f(z) before its quotient is complete and the MSMs run on streams of their own).
  (c) bbgpu_srs_lagrange_check without LOCATE against two device MSMs of n scalars in flight, over the same two handles (both child), at 2^16 and 2^20 rows.
No ratio is asserted: the lines say which leg's median is lower and whether the gap exceeds the spread (the slower leg's interquartile range).
Usage: make the parent's library once (barretenberg_amd/csrc: `make variant NAME=parent` in a checkout of the parent, copied to
barretenberg_amd/_variants/libbbgpu_parent.so), then  python tools/lagrange_open_bench.py [--pairs 21] [--parent-lib PATH] [--out PATH]"""
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
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def stats(ts):
    q = statistics.quantiles(ts, n=4)
    return dict(med=statistics.median(ts), lo=min(ts), hi=max(ts), iqr=q[2] - q[0])


def show(name, ts):
    s = stats(ts)
    return "%s %8.3f (min %8.3f max %8.3f iqr %6.3f)" % (name, s["med"], s["lo"], s["hi"], s["iqr"])


def timed(call):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


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


def line(what, name_a, ta, name_b, tb):
    sa, sb = stats(ta), stats(tb)
    lower, gap, spread = (name_a, sb["med"] - sa["med"], sb["iqr"]) if sa["med"] <= sb["med"] else (name_b, sa["med"] - sb["med"], sa["iqr"])
    say("%s  %s  %s  lower median: %s by %.3f ms (%s the spread of %.3f)"
        % (what, show(name_a, ta), show(name_b, tb), lower, gap, "more than" if gap > spread else "within", spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=21)
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lagrange_open.txt"))
    args = ap.parse_args()
    import torch
    from barretenberg_amd import BbGpu
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s (see the usage)" % args.parent_lib)
    child = BbGpu(device=0)
    os.environ["BBGPU_LIB"] = args.parent_lib
    parent = BbGpu(device=0)
    del os.environ["BBGPU_LIB"]
    say("# child %s, parent %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of %d alternating pairs after a warm pair"
        % (child.version(), parent.version(), args.pairs))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x1A60BE)
    x = np.array([0x1234567, 0x89ABCDE, 0xF012345, 0x6789AB], dtype=np.uint64)  # any secret: a string nobody uses
    z = np.array([0x0F1E2D3C4B5A6978, 0x1122334455667788, 0x99AABBCCDDEEFF00, 0x0123456789ABCDEF], dtype=np.uint64)
    for n in (1 << 16, 1 << 20):
        h_child, h_parent = child.srs_generate(x, n), parent.srs_generate(x, n)
        h_lagrange, _, _ = child.srs_lagrange(h_child, n)
        for batch in (1, 8):
            v = torch.randint(-(1 << 63), (1 << 63) - 1, (batch * n, 4), dtype=torch.int64, device="cuda", generator=gen)
            c, q, qc = v.clone(), torch.empty_like(v), torch.empty_like(v)
            at = [b * n * 32 for b in range(batch)]

            def evaluate_values():
                child.evaluate_lagrange_device(v.data_ptr(), n, z, batch=batch)

            def evaluate_transform():
                parent.ntt_device_batch(c.data_ptr(), n, batch, "ifft")
                for o in at:
                    parent.evaluate_device(c.data_ptr() + o, n, z)

            def open_values():
                child.kate_opening_lagrange_device(v.data_ptr(), q.data_ptr(), n, z, batch=batch)

            def open_transform():
                parent.ntt_device_batch(c.data_ptr(), n, batch, "ifft")
                for o in at:
                    parent.compute_kate_opening_coefficients_device(c.data_ptr() + o, qc.data_ptr() + o, n, z)

            def open_values_commit():
                open_values()
                for o in at:
                    child.msm_device(h_lagrange, q.data_ptr() + o, n)

            def open_transform_commit():
                open_transform()
                torch.cuda.synchronize()  # bbgpu_kate_opening_device returns f(z) before its quotient is complete, and the MSMs run on streams of their own
                for o in at:
                    parent.msm_device(h_parent, qc.data_ptr() + o, n)
            tag = "n 2^%d batch %d" % (n.bit_length() - 1, batch)
            ta, tb = pairs(args.pairs, evaluate_values, evaluate_transform)
            line("(a) evaluate      %s" % tag, "values", ta, "transform", tb)
            ta, tb = pairs(args.pairs, open_values, open_transform)
            line("(b) open          %s" % tag, "values", ta, "transform", tb)
            ta, tb = pairs(args.pairs, open_values_commit, open_transform_commit)
            line("(b) open + commit %s" % tag, "values", ta, "transform", tb)
            del v, c, q, qc
        s = torch.randint(0, (1 << 62), (n, 4), dtype=torch.int64, device="cuda", generator=gen)  # below 2^254 < 2r: the top limb stays below 2^62

        def check():
            assert child.srs_lagrange_check(h_lagrange, h_child, n, seed=SEED).ok

        def two_msms():
            ta = child.msm_device_async(h_lagrange, s.data_ptr(), n)
            tb = child.msm_device_async(h_child, s.data_ptr(), n)
            child.msm_wait(ta)
            child.msm_wait(tb)
        ta, tb = pairs(args.pairs, check, two_msms)
        line("(c) check         n 2^%d        " % (n.bit_length() - 1), "check", ta, "two MSMs", tb)
        child.srs_release(h_lagrange)
        child.srs_release(h_child)
        parent.srs_release(h_parent)
        del s
    child.shutdown()
    parent.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
