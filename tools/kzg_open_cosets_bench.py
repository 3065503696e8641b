"""What the cell proofs of a polynomial -- one KZG proof per coset of l points of its domain -- cost through bbgpu_kzg_open_cosets_device, against the path
a caller had before (profiles/kzg_open_cosets.txt is this tool's output): one process on one MI355X, every leg warm, the two legs of a cell alternating
inside every pair (the order swapped from pair to pair).  Wall milliseconds per call around the C entries, Python binding included, each leg ended by a
device synchronise; the legacy default stream; random coefficients; a generated string nobody uses.
  open-cosets  one bbgpu_kzg_open_cosets_device call: batch polynomials, all n / l cell proofs of each, read back to the host.
  open-all     one bbgpu_kzg_open_all_device call at the same n and batch: all n single proofs, read back to the host -- the first half of the old path.
               Its second half, an l-point MSM per cell on the host, is NOT timed and not charged: the comparison favours the old path.
(n, l) = (2^12, 64), (2^16, 64), (2^16, 4) with batch 1 and 16, (2^20, 64) with batch 1.  bbgpu_kzg_open_cosets_setup is timed alone (setup + release, not
paired).  The per-kernel device times of one call per leg and cell come from bbgpu_set_timing; both entries run k_open_cosets_sum over the same 2 n
ladders per polynomial, the open-all one at coset size 1 where its tree has no level, so the difference of the two is the tree of additions across lanes.
No ratio is asserted: the lines say which leg's median is lower and whether the gap exceeds the spread, taken as the larger of the two legs' full ranges
(max - min).
--head FILE puts the lines of FILE in front of the output (the compiler's resource remarks for csrc/kzg_open_cosets.hip, which no run on the GPU can make).
Usage: python tools/kzg_open_cosets_bench.py [--pairs 9] [--head FILE] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.lagrange_open_bench import LINES, pairs, say, show, stats, timed  # noqa: E402  (the same clock, pairing and report lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_open_cosets.txt"))
    args = ap.parse_args()
    import torch
    from barretenberg_amd import BbGpu
    if args.head:
        with open(args.head) as fh:
            for text in fh.read().splitlines():
                say(text)
    lib = BbGpu(device=0)
    say("# %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of alternating pairs after a warm pair" % lib.version())
    say("# open-all: the n single proofs only; the l-point host fold per cell that the old path needs on top is not timed")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xC05E7)
    x = np.array([0x1234567, 0x89ABCDE, 0xF012345, 0x6789AB], dtype=np.uint64)  # any secret: a string nobody uses
    for lg, cosets, batches, npairs in ((12, (64,), (1, 16), args.pairs), (16, (64, 4), (1, 16), args.pairs), (20, (64,), (1,), max(3, args.pairs // 3))):
        n = 1 << lg
        h = lib.srs_generate(x, n)
        single = lib.kzg_open_all_setup(h, n)
        c = torch.randint(-(1 << 63), (1 << 63) - 1, (max(batches) * n, 4), dtype=torch.int64, device="cuda", generator=gen)
        out_all = np.zeros((max(batches), n, 8), dtype=np.uint64)
        for l in cosets:
            m = n // l
            ts = [timed(lambda: lib.kzg_open_cosets_release(lib.kzg_open_cosets_setup(h, n, l))) for _ in range(4)]
            say("setup + release n 2^%d l %2d  %s" % (lg, l, show("wall", ts[1:])))
            setup = lib.kzg_open_cosets_setup(h, n, l)
            out = np.zeros((max(batches), m, 8), dtype=np.uint64)
            for batch in batches:
                ta, tb = pairs(npairs, lambda: lib.kzg_open_cosets_device(setup, c.data_ptr(), n, l, batch=batch, out=out[:batch]),
                               lambda: lib.kzg_open_all_device(single, c.data_ptr(), n, batch=batch, out=out_all[:batch]))
                sa, sb = stats(ta), stats(tb)
                lower, gap = ("open-cosets", sb["med"] - sa["med"]) if sa["med"] <= sb["med"] else ("open-all", sa["med"] - sb["med"])
                spread = max(sa["hi"] - sa["lo"], sb["hi"] - sb["lo"])
                say("n 2^%d l %2d batch %2d (%d pairs)  %s  %s  lower median: %s by %.3f ms (%s the spread of %.3f)"
                    % (lg, l, batch, npairs, show("open-cosets", ta), show("open-all", tb), lower, gap, "more than" if gap > spread else "within", spread))
                lib.set_timing(1)
                lib.kzg_open_cosets_device(setup, c.data_ptr(), n, l, batch=batch, out=out[:batch])
                ms = lib.last_timing()
                lib.kzg_open_all_device(single, c.data_ptr(), n, batch=batch, out=out_all[:batch])
                ms_all = lib.last_timing()
                lib.set_timing(0)
                say("n 2^%d l %2d batch %2d  open-cosets device ms: sum %.3f, inverse stages %.3f, gather + forward stages %.3f, finish %.3f" % ((lg, l, batch) + tuple(ms)))
                say("n 2^%d l %2d batch %2d  open-all    device ms: sum (l = 1) %.3f, inverse stages %.3f, gather + forward stages %.3f, finish %.3f; "
                    "k_open_cosets_sum at this l - at l = 1, the same %d ladders: %+.3f ms" % ((lg, l, batch) + tuple(ms_all) + (2 * n * batch, ms[0] - ms_all[0])))
            lib.kzg_open_cosets_release(setup)
        lib.kzg_open_all_release(single)
        lib.srs_release(h)
        del c
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
