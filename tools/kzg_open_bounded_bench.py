"""What bbgpu_kzg_open_cosets_device costs over a setup with a degree bound d = n / 2 (bbgpu_kzg_open_cosets_setup_bounded) against the same entry over a
setup without one, fed the same coefficients zero-padded to n (profiles/kzg_open_bounded.txt is this tool's output): one process on one MI355X, every leg
warm, the two legs of a cell alternating inside every pair (the order swapped from pair to pair).  Wall milliseconds per call around the C entry, Python
binding included, each leg ended by a device synchronise, proofs read back to the host; the legacy default stream; random coefficients below d, zeros
from d on; a generated string nobody uses.
  bounded    one call over the bounded setup: stride n, coefficients [0, d) read.
  unbounded  one call over bbgpu_kzg_open_cosets_setup(h, n, l) on the same buffer.
(n, l) = (2^12, 64) and (2^16, 64) with batch 1 and 16, (2^20, 64) with batch 1.  Both setups are timed alone (setup + release, not paired).  The
per-kernel device times of one call per leg come from bbgpu_set_timing.  The proofs of the two legs are compared once per shape.  No ratio is asserted:
the lines say which leg's median is lower and whether the gap exceeds the spread, taken as the larger of the two legs' full ranges (max - min).
NOT timed: other ratios d / n, l < 64, the host twin.
--head FILE puts the lines of FILE in front of the output (the compiler's resource remarks for csrc/kzg_open_cosets.hip, which no run on the GPU can make).
Usage: python tools/kzg_open_bounded_bench.py [--pairs 9] [--head FILE] [--out PATH]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_open_bounded.txt"))
    args = ap.parse_args()
    import torch
    from barretenberg_amd import BbGpu
    if args.head:
        with open(args.head) as fh:
            for text in fh.read().splitlines():
                say(text)
    lib = BbGpu(device=0)
    say("# %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of alternating pairs after a warm pair" % lib.version())
    say("# bounded: d = n / 2; unbounded: the same buffer (zeros from d on) over a setup without a bound; proofs read back in both")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xB0D)
    x = np.array([0x1234567, 0x89ABCDE, 0xF012345, 0x6789AB], dtype=np.uint64)  # any secret: a string nobody uses
    l = 64
    for lg, batches, npairs in ((12, (1, 16), args.pairs), (16, (1, 16), args.pairs), (20, (1,), max(3, args.pairs // 3))):
        n = 1 << lg
        d, m = n // 2, n // l
        h = lib.srs_generate(x, n)
        c = torch.randint(-(1 << 63), (1 << 63) - 1, (max(batches), n, 4), dtype=torch.int64, device="cuda", generator=gen)
        c[:, d:] = 0
        for name, bound in (("bounded  ", d), ("unbounded", None)):
            ts = [timed(lambda: lib.kzg_open_cosets_release(lib.kzg_open_cosets_setup(h, n, l, degree_bound=bound))) for _ in range(4)]
            say("setup + release n 2^%d l %2d %s  %s" % (lg, l, name, show("wall", ts[1:])))
        new, old = lib.kzg_open_cosets_setup(h, n, l, degree_bound=d), lib.kzg_open_cosets_setup(h, n, l)
        out_new, out_old = (np.zeros((max(batches), m, 8), dtype=np.uint64) for _ in range(2))
        for batch in batches:
            ta, tb = pairs(npairs, lambda: lib.kzg_open_cosets_device(new, c.data_ptr(), n, l, batch=batch, out=out_new[:batch]),
                           lambda: lib.kzg_open_cosets_device(old, c.data_ptr(), n, l, batch=batch, out=out_old[:batch]))
            same = np.array_equal(out_new[:batch], out_old[:batch])
            sa, sb = stats(ta), stats(tb)
            lower, gap = ("bounded", sb["med"] - sa["med"]) if sa["med"] <= sb["med"] else ("unbounded", sa["med"] - sb["med"])
            spread = max(sa["hi"] - sa["lo"], sb["hi"] - sb["lo"])
            say("n 2^%d l %2d batch %2d (%d pairs)  %s  %s  lower median: %s by %.3f ms (%s the spread of %.3f); proofs equal: %s"
                % (lg, l, batch, npairs, show("bounded", ta), show("unbounded", tb), lower, gap, "more than" if gap > spread else "within", spread, same))
            lib.set_timing(1)
            for name, setup, out in (("bounded  ", new, out_new), ("unbounded", old, out_old)):
                lib.kzg_open_cosets_device(setup, c.data_ptr(), n, l, batch=batch, out=out[:batch])
                say("n 2^%d l %2d batch %2d  %s device ms: sum %.3f, inverse stages %.3f, gather + forward stages %.3f, finish %.3f"
                    % ((lg, l, batch, name) + tuple(lib.last_timing())))
            lib.set_timing(0)
        lib.kzg_open_cosets_release(new)
        lib.kzg_open_cosets_release(old)
        lib.srs_release(h)
        del c
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
