"""What bbgpu_g1_recover_each costs -- erasure decoding of columns of curve points whose row sets differ (profiles/g1_recover_each.txt is this tool's
output): one process on one MI355X, every leg warm, the two legs of a line alternating inside every pair (the order swapped from pair to pair), medians of
--pairs pairs.  Wall milliseconds per leg around the C entries, Python binding and the copies of the points across the link included, each leg ended by a
device synchronise; the legacy default stream; the output buffers made once.  The columns are honest codewords of degree < n / 2 as
tools/g1_recover_bench.py makes them, and half the rows of every column are missing (degree bound n / 2: no redundancy).  The rule of the open-cosets block:
a median counts as lower only if it is lower by more than the full range (max - min) of either leg.
  each   (a) ONE bbgpu_g1_recover_each call over `batch` columns, a different seeded random half of the rows missing in each, beside the only route there was
         before: one bbgpu_g1_recover call per DISTINCT set (columns that drew the same set share a call), the same process, at (n, batch) = (8, 65),
         (64, 65), (512, 65), (4096, 16).
  same   (b) the SAME set for all columns (every other row): this entry beside one bbgpu_g1_recover call at the same shapes -- the price of the per-column
         lists and tables.
  vanish (c) bbgpu_last_timing index 0 (k_g1_roots and k_g1_vanish_cols) at (4096, 256) with a different random half missing per column, beside its
         product count sum_b 2 mu_b n at the 150 Gmul/s of csrc/fe_mont_gfx950.h.  No ratio is asserted and nothing is tuned to it.
--head FILE puts the lines of FILE in front of the output (the compiler's resource remarks).  --only KIND[,KIND] runs some of each, same, vanish.
Usage: python tools/g1_recover_each_bench.py [--pairs 9] [--only each,same,vanish] [--head FILE] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.g1_recover_bench import codewords, range_rule  # noqa: E402  (the same columns and the same rule)
from tools.lagrange_open_bench import LINES, pairs, say, show, stats  # noqa: E402  (the same clock, pairing and report lines)

SHAPES = ((8, 65), (64, 65), (512, 65), (4096, 16))
VANISH = (4096, 256)
GMULS = 150e9  # field products per second of csrc/fe_mont_gfx950.h


def random_halves(n, batch, seed):
    """per column the ascending rows that are present: a seeded random half"""
    rng = np.random.default_rng([0x61EE, n, batch, seed])
    return [np.sort(rng.permutation(n)[:n // 2]).astype(np.uint32) for _ in range(batch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--only", default="each,same,vanish")
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_recover_each.txt"))
    args = ap.parse_args()
    from barretenberg_amd import BbGpu
    if args.head:
        with open(args.head) as fh:
            for text in fh.read().splitlines():
                say(text)
    lib = BbGpu(device=0)
    say("# %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of %d alternating pairs after a warm pair" %
        (lib.version(), args.pairs))
    only = args.only.split(",")
    x = np.array([0x0123456789ABCDEF, 0x0F1E2D3C4B5A6978, 0x7766554433221100, 0x0011223344556677], dtype=np.uint64)
    h, table = lib.srs_generate(x, 1 << 16, want_host_table=True)
    pool = np.ascontiguousarray(table[0::2])  # 2^16 distinct affine points on the curve, canonical

    for n, batch in SHAPES if ("each" in only or "same" in only) else ():
        d = n // 2
        values = codewords(lib, pool, n, d, batch)
        out = np.zeros((batch, n, 8), dtype=np.uint64)
        if "each" in only:
            rows = random_halves(n, batch, 1)
            flat = np.ascontiguousarray(np.concatenate([values[b, r] for b, r in enumerate(rows)]))
            groups = {}
            for b, r in enumerate(rows):
                groups.setdefault(r.tobytes(), []).append(b)
            calls = [(rows[cols[0]], np.ascontiguousarray(values[cols][:, rows[cols[0]]]), np.zeros((len(cols), n, 8), dtype=np.uint64), cols)
                     for cols in groups.values()]

            def each(rows=rows, flat=flat, n=n, d=d, out=out):
                return lib.g1_recover_each(rows, flat, n, d, out=out)

            def one_by_one(calls=calls, n=n, d=d):
                for r, pts, into, cols in calls:
                    lib.g1_recover(r, pts, n, d, batch=len(cols), out=into)
            got, rep, _ = each()
            one_by_one()
            if not (np.array_equal(got, values) and rep["consistent"] == 1 and all(np.array_equal(into, values[cols]) for _, _, into, cols in calls)):
                sys.exit("n %d batch %d: a recovery is wrong" % (n, batch))
            lib.set_timing(1)
            each()
            ms = lib.last_timing()
            lib.set_timing(0)
            ta, tb = pairs(args.pairs, each, one_by_one)
            say("(a) n %4d batch %2d, a different random half missing per column, %2d distinct sets  %s  %s  ratio of medians %.1f  %s; device ms of the one "
                "call: roots + vanishing values %.3f, load + IFFT %.3f, shift .. verdict %.3f, FFT + finish %.3f"
                % (n, batch, len(calls), show("g1_recover_each, 1 call", ta), show("g1_recover, %d calls" % len(calls), tb), stats(tb)["med"] / stats(ta)["med"],
                   range_rule("each", ta, "one by one", tb), ms[0], ms[1], ms[2], ms[3]))
        if "same" in only:
            shared = np.arange(0, n, 2, dtype=np.uint32)
            points = np.ascontiguousarray(values[:, shared])
            lists = [shared] * batch
            other = np.zeros((batch, n, 8), dtype=np.uint64)

            def each_same(lists=lists, points=points, n=n, d=d, out=out):
                return lib.g1_recover_each(lists, points, n, d, out=out)

            def same(shared=shared, points=points, n=n, d=d, batch=batch, other=other):
                return lib.g1_recover(shared, points, n, d, batch=batch, out=other)
            if not (np.array_equal(each_same()[0], values) and np.array_equal(same()[0], values)):
                sys.exit("n %d batch %d, one set: a recovery is wrong" % (n, batch))
            ta, tb = pairs(args.pairs, each_same, same)
            say("(b) n %4d batch %2d, every other row missing in every column  %s  %s  %s"
                % (n, batch, show("g1_recover_each", ta), show("g1_recover", tb), range_rule("each", ta, "same-set entry", tb)))

    if "vanish" in only:
        n, batch = VANISH
        d = n // 2
        values = np.ascontiguousarray(np.tile(codewords(lib, pool, n, d, 16), (batch // 16, 1, 1)))  # 16 columns, repeated: the time does not depend on them
        rows = random_halves(n, batch, 2)
        flat = np.ascontiguousarray(np.concatenate([values[b, r] for b, r in enumerate(rows)]))
        out = np.zeros((batch, n, 8), dtype=np.uint64)
        got, rep, _ = lib.g1_recover_each(rows, flat, n, d, out=out)
        if not (np.array_equal(got, values) and rep["consistent"] == 1):
            sys.exit("n %d batch %d: the recovery is wrong" % (n, batch))
        lib.set_timing(1)
        ts = []
        for _ in range(3):
            lib.g1_recover_each(rows, flat, n, d, out=out)
            ts.append(lib.last_timing())
        lib.set_timing(0)
        t0 = float(np.median([t[0] for t in ts]))
        products = sum(2 * (n - len(r)) * n for r in rows)
        model = products / GMULS * 1e3
        say("(c) n %d batch %d, a different random half missing per column: bbgpu_last_timing index 0 (k_g1_roots + k_g1_vanish_cols) %.3f ms (min %.3f max %.3f of "
            "3 calls); sum_b 2 mu_b n = %d products = %.3f ms at 150 Gmul/s: %.2f times that; the other indices of the last call: load + IFFT %.1f, shift .. "
            "verdict %.1f, FFT + finish %.1f ms"
            % (n, batch, t0, min(t[0] for t in ts), max(t[0] for t in ts), products, model, t0 / model, ts[-1][1], ts[-1][2], ts[-1][3]))
    say("# NOT timed: the host twin; the host's part of a call on its own (the curve test of every point, the lists of missing rows); the batch inversion over "
        "batch x n values on its own (it lies between indices 0 and 1 and is in neither); columns that miss few rows beside columns that miss many in one "
        "call; n < 4096 at batch x n = 2^20; any shape on a non-default stream")
    lib.srs_release(h)
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
