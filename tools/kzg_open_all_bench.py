"""What opening a polynomial at every point of its domain costs through bbgpu_kzg_open_all_device, against the path a caller had before
(profiles/kzg_open_all.txt is this tool's output): one process on one MI355X, every leg warm, the two legs of a cell alternating inside every pair (the
order swapped from pair to pair).  Wall milliseconds per call around the C entries, Python binding included, each leg ended by a device synchronise; the
legacy default stream; random coefficients; a generated string nobody uses.
  open-all    one bbgpu_kzg_open_all_device call: batch polynomials, all n proofs of each, read back to the host.
  per-point   bbgpu_kate_opening_device at omega^i, a device synchronise (the MSM runs on a stream of its own), then bbgpu_msm_g1_device over the same SRS
              handle, for ONE polynomial at a SAMPLE of 256 points (fixed indices).  The leg's time is that of the 256 points; the report scales it by
              n / 256 to all n points of one polynomial, and by the batch to the batch -- an extrapolation, marked as such on every line.
n = 2^12 and 2^16 with batch 1 and 16, n = 2^20 with batch 1.  bbgpu_kzg_open_all_setup is timed alone (setup + release, not paired).  The per-kernel
device times of one call per cell come from bbgpu_set_timing; the first is k_open_cosets_sum of csrc/kzg_open_cosets.hip, which at coset size 1 multiplies
each row by its own scalar and adds nothing.  No ratio is asserted: the lines say which leg's median is lower and whether the gap exceeds the spread (the
slower leg's interquartile range).
Usage: python tools/kzg_open_all_bench.py [--pairs 9] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from barretenberg_amd.plonk import FR_MODULUS, to_montgomery_limbs  # noqa: E402
from tools.lagrange_open_bench import LINES, pairs, say, show, stats, timed  # noqa: E402  (the same clock, pairing and report lines)

MONT_INV = pow(1 << 256, -1, FR_MODULUS)
ROOT28 = 0x1860EF942963F9E756452AC01EB203D8A22BF3742445FFD6636E735580D13D9C * MONT_INV % FR_MODULUS  # the 2^28-th root of unity, out of its Montgomery form
SAMPLE = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_open_all.txt"))
    args = ap.parse_args()
    import torch
    from barretenberg_amd import BbGpu
    lib = BbGpu(device=0)
    say("# %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of alternating pairs after a warm pair" % lib.version())
    say("# per-point: %d sampled points of one polynomial per leg; 'scaled' = that time x n / %d x batch, an extrapolation" % (SAMPLE, SAMPLE))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x0A11)
    x = np.array([0x1234567, 0x89ABCDE, 0xF012345, 0x6789AB], dtype=np.uint64)  # any secret: a string nobody uses
    for lg, batches, npairs in ((12, (1, 16), args.pairs), (16, (1, 16), args.pairs), (20, (1,), max(3, args.pairs // 3))):
        n = 1 << lg
        w = pow(ROOT28, 1 << (28 - lg), FR_MODULUS)
        picks = [(k * 2654435761 + k) % n for k in range(SAMPLE)]
        zs = to_montgomery_limbs([pow(w, i, FR_MODULUS) for i in picks])
        h = lib.srs_generate(x, n)
        ts = []
        for k in range(4):
            ts.append(timed(lambda: lib.kzg_open_all_release(lib.kzg_open_all_setup(h, n))))
        say("setup + release n 2^%d  %s" % (lg, show("wall", ts[1:])))
        setup = lib.kzg_open_all_setup(h, n)
        c = torch.randint(-(1 << 63), (1 << 63) - 1, (max(batches) * n, 4), dtype=torch.int64, device="cuda", generator=gen)
        q = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        out = np.zeros((max(batches), n, 8), dtype=np.uint64)

        def per_point():
            for z in zs:
                lib.compute_kate_opening_coefficients_device(c.data_ptr(), q.data_ptr(), n, z)
                torch.cuda.synchronize()
                lib.msm_device(h, q.data_ptr(), n)
        for batch in batches:
            ta, tb = pairs(npairs, lambda: lib.kzg_open_all_device(setup, c.data_ptr(), n, batch=batch, out=out[:batch]), per_point)
            sa, sb = stats(ta), stats(tb)
            scale = n / SAMPLE * batch
            scaled = sb["med"] * scale
            lower, gap, spread = ("open-all", scaled - sa["med"], sb["iqr"] * scale) if sa["med"] <= scaled else ("per-point", sa["med"] - scaled, sa["iqr"])
            say("n 2^%d batch %2d (%d pairs)  %s  %s  per-point scaled to %d x %d points: %.1f ms  lower median: %s by %.1f ms (%s the spread of %.1f)"
                % (lg, batch, npairs, show("open-all", ta), show("per-point, %d points" % SAMPLE, tb), batch, n, scaled, lower, gap,
                   "more than" if gap > spread else "within", spread))
            lib.set_timing(1)
            lib.kzg_open_all_device(setup, c.data_ptr(), n, batch=batch, out=out[:batch])
            ms = lib.last_timing()
            lib.set_timing(0)
            say("n 2^%d batch %2d  device ms: sum (l = 1) %.3f, inverse stages %.3f, gather + forward stages %.3f, finish %.3f" % ((lg, batch) + tuple(ms)))
        lib.kzg_open_all_release(setup)
        lib.srs_release(h)
        del c, q
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
