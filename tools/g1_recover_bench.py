"""What bbgpu_g1_ntt and bbgpu_g1_recover cost -- transforms and erasure decoding on columns of curve points (profiles/g1_recover.txt is this tool's
output): one process on one MI355X, every leg warm, the two legs of a line alternating inside every pair (the order swapped from pair to pair), medians of
--pairs pairs.  Wall milliseconds per call around the C entries, Python binding and the copies of the points across the link included, each leg ended by a
device synchronise; the legacy default stream; the output buffer made once.  The columns are honest codewords: d points of a resident string as
coefficients, infinity above, their values by bbgpu_g1_ntt.
  stage    (a) k_g1_stage_cols beside the parent's mapping -- k_lagrange_stage with the column in blockIdx.y, through bbgpu_g1_set_stage_mapping(1) -- the
           same forward transforms by bbgpu_g1_ntt at (n, batch) = (8, 4096), (512, 65), (2^16, 1).  The rule of the open-cosets block: a mapping wins a
           shape only if its median is lower by more than the full range (max - min) of either leg.
  recover  (b) bbgpu_g1_recover at (n, batch, missing) = (8, 65, 4), (512, 65, 256), (4096, 16, 2048), degree bound n - missing, beside 4 + 4 log2 n times
           the latency of one ladder-bearing launch, measured in the same run as the device time of the load and the one-stage transform of a call at
           (2, 1) (one wave, one ladder; the stage at n = 2 is position 0 and runs none).  Device times from bbgpu_set_timing.  No ratio is asserted.
  producer (c) at (512, 65, 256): the decode beside producing the same 256 rows' proofs with bbgpu_kzg_open_cosets_device at (2^12, 64), 16 calls of batch 16.
--head FILE puts the lines of FILE in front of the output (the compiler's resource remarks).  --only KIND[,KIND] runs some of stage, recover, producer.
Usage: python tools/g1_recover_bench.py [--pairs 9] [--only stage,recover,producer] [--head FILE] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.lagrange_open_bench import LINES, pairs, say, show, stats  # noqa: E402  (the same clock, pairing and report lines)

STAGE = ((8, 4096), (64, 512), (64, 8192), (128, 256), (128, 4096), (512, 65), (1 << 16, 1))
RECOVER = ((8, 65, 4), (512, 65, 256), (4096, 16, 2048))
INF = np.array([0, 0, 0, 0, 0, 0, 0, 1 << 63], dtype=np.uint64)


def codewords(lib, pool, n, d, batch):
    """(batch, n, 8): column b = the values of the "polynomial" whose d coefficients are points of the pool"""
    coeffs = np.empty((batch, n, 8), dtype=np.uint64)
    coeffs[:] = INF
    take = np.arange(batch * d) % pool.shape[0]
    coeffs[:, :d] = pool[take].reshape(batch, d, 8)
    return lib.g1_ntt(coeffs, n, "fft", batch=batch)


def range_rule(name_a, ta, name_b, tb):
    sa, sb = stats(ta), stats(tb)
    full = max(sa["hi"] - sa["lo"], sb["hi"] - sb["lo"])
    gap = abs(sa["med"] - sb["med"])
    lower = name_a if sa["med"] <= sb["med"] else name_b
    return "lower median: %s by %.3f ms, %s the full range %.3f of either leg" % (lower, gap, "more than" if gap > full else "within", full)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--only", default="stage,recover,producer")
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g1_recover.txt"))
    args = ap.parse_args()
    import torch
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
    pool = np.ascontiguousarray(table[0::2])  # 2^16 distinct affine points on the curve, canonical: no column repeats a point

    for n, batch in STAGE if "stage" in only else ():
        points = codewords(lib, pool, n, n, batch)
        out = np.zeros((batch, n, 8), dtype=np.uint64)

        def leg(mapping):
            def run():
                lib.g1_set_stage_mapping(mapping)
                try:
                    return lib.g1_ntt(points, n, "fft", batch=batch, out=out)
                finally:
                    lib.g1_set_stage_mapping(0)
            return run
        a = leg(2)().copy()
        if not np.array_equal(a, leg(1)()):
            sys.exit("n %d batch %d: the two mappings disagree" % (n, batch))
        ta, tb = pairs(args.pairs, leg(2), leg(1))
        say("(a) g1_ntt forward, n %5d batch %4d  %s  %s  %s" % (n, batch, show("cols", ta), show("blockIdx.y", tb), range_rule("cols", ta, "blockIdx.y", tb)))

    ladder = None
    if "recover" in only or "producer" in only:
        tiny = codewords(lib, pool, 2, 1, 1)
        lib.set_timing(1)
        ts = []
        for _ in range(args.pairs + 1):
            lib.g1_recover(np.array([1], dtype=np.uint32), tiny[:, 1], 2, 1)
            ts.append(lib.last_timing()[1])
        lib.set_timing(0)
        ladder = float(np.median(ts[1:]))
        say("# one ladder-bearing launch: %.4f ms (min %.4f max %.4f) -- device time of k_g1_load with one ladder and the one stage of n = 2, which runs none, "
            "at (2, 1), median of %d calls" % (ladder, min(ts[1:]), max(ts[1:]), args.pairs))

    decode512 = None
    for n, batch, mu in RECOVER if ("recover" in only or "producer" in only) else ():
        d = n - mu
        values = codewords(lib, pool, n, d, batch)
        rows = np.arange(0, n, 2, dtype=np.uint32) if 2 * mu == n else np.arange(n - mu, dtype=np.uint32)  # every other row, or the first n - mu
        points = np.ascontiguousarray(values[:, rows])
        out = np.zeros((batch, n, 8), dtype=np.uint64)
        call = lambda rows=rows, points=points, n=n, d=d, batch=batch, out=out: lib.g1_recover(rows, points, n, d, batch=batch, out=out)  # noqa: E731
        got, rep = call()
        if not (np.array_equal(got, values) and rep["consistent"] == 1):
            sys.exit("n %d batch %d missing %d: the recovery is wrong" % (n, batch, mu))
        lib.set_timing(1)
        call()
        ms = lib.last_timing()
        lib.set_timing(0)
        ta, tb = pairs(args.pairs, call, call)
        wall = ta + tb
        launches = 4 + 4 * (n.bit_length() - 1)
        dev = ms[1] + ms[2] + ms[3]
        say("(b) g1_recover n %4d batch %2d missing %4d (d %d)  %s  device ms: vanishing values %.3f, load + IFFT %.3f, shift .. verdict %.3f, FFT + finish %.3f "
            "(finish alone %.3f); %d ladder-bearing launches x %.4f = %.3f ms: device %.3f is %.2f times that, wall %.2f times"
            % (n, batch, mu, d, show("wall", wall), ms[0], ms[1], ms[2], ms[3], ms[4], launches, ladder, launches * ladder, dev, dev / (launches * ladder),
               stats(wall)["med"] / (launches * ladder)))
        if (n, batch, mu) == (512, 65, 256):
            decode512 = call

    if "producer" in only and decode512 is not None:
        pn, pl, pb = 1 << 12, 64, 16
        setup = lib.kzg_open_cosets_setup(h, pn, pl)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0x61EC)
        d_coeffs = torch.randint(-(1 << 63), (1 << 63) - 1, (pb, pn, 4), dtype=torch.int64, device="cuda", generator=gen)
        proofs = np.zeros((pb, pn // pl, 8), dtype=np.uint64)

        def produce():
            for _ in range(256 // pb):
                lib.kzg_open_cosets_device(setup, d_coeffs.data_ptr(), pn, pl, batch=pb, out=proofs)
        ta, tb = pairs(args.pairs, decode512, produce)
        say("(c) the proofs of 256 extension rows of a (2^12, 64) layout: %s  %s  (the decode also returns the 256 commitments; the producer needs the rows' data)"
            % (show("g1_recover (512, 65, 256)", ta), show("kzg_open_cosets_device, 16 calls of batch 16", tb)))
        lib.kzg_open_cosets_release(setup)
    lib.srs_release(h)
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
