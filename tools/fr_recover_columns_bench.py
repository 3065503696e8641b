"""What bbgpu_fr_recover_columns_device costs -- erasure decoding down the columns of a resident matrix of field elements, a tile of whole columns
decoded in LDS (profiles/fr_recover_columns.txt is this tool's output): one process on one MI355X, every leg warm, the two legs of a line alternating
inside every pair (the order swapped from pair to pair), medians of --pairs pairs.  Wall milliseconds per leg around the C entries, the Python binding
included, each leg ended by a device synchronise; the legacy default stream; no first_bad_out (one 16-byte read-back per call).  The matrix is made on
the device: seeded coefficient rows [0, d), zero rows above, bbgpu_fr_ntt_columns_device down the columns -- honest codewords of degree < d = rows / 2 --
and half the rows of every set are missing, a different seeded random half per set (no redundancy).  A call writes the missing rows with the values they
had, so the same matrix serves every repetition; it is compared with its first state after the last one.
At (rows, width, sets) = (512, 2^16, 1), (512, 2^16, 1024), (64, 2^16, 64), (8, 2^18, 1), (2048, 2^12, 1) the call stands beside two yardsticks that are
not the code under test:
  (a) the decode kernel's own product count, (4 (log2 rows) / 2 + 4) rows width, at the 150 Gmul/s of csrc/fe_mont_gfx950.h;
  (b) four bbgpu_ntt_device_batch calls over the same number of elements, arranged as 64 transforms of rows width / 64: existing code that runs more
      stages per element, an upper reference and not a target.
Device ms: bbgpu_last_timing of the call (index 0 the roots, the vanishing values, their inversion and the tables; index 1 the decode kernel), and
events around the four transforms.  No ratio is asserted and nothing is tuned to one.
--head FILE puts the lines of FILE in front of the output (the compiler's resource remarks).
Usage: python tools/fr_recover_columns_bench.py [--pairs 9] [--head FILE] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.lagrange_open_bench import LINES, pairs, say, show  # noqa: E402  (the same clock, pairing and report lines)

SHAPES = ((512, 1 << 16, 1), (512, 1 << 16, 1024), (64, 1 << 16, 64), (8, 1 << 18, 1), (2048, 1 << 12, 1))
GMULS = 150e9  # field products per second of csrc/fe_mont_gfx950.h


def random_halves(rows, sets, seed):
    """per set the ascending rows that are present: a seeded random half"""
    rng = np.random.default_rng([0xF2C0, rows, sets, seed])
    return [np.sort(rng.permutation(rows)[:rows // 2]).astype(np.uint32) for _ in range(sets)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fr_recover_columns.txt"))
    args = ap.parse_args()
    import torch
    from barretenberg_amd import BbGpu
    if args.head:
        with open(args.head) as fh:
            for text in fh.read().splitlines():
                say(text)
    lib = BbGpu(device=0)
    say("# %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of %d alternating pairs after a warm pair; device ms: "
        "medians over the same calls" % (lib.version(), args.pairs))
    for rows, width, sets in SHAPES:
        d, total = rows // 2, rows * width
        gen = torch.Generator(device="cuda").manual_seed(rows * 31 + sets)
        m = torch.randint(0, 1 << 62, (rows, width, 4), dtype=torch.int64, device="cuda", generator=gen)
        m[:, :, 3] &= (1 << 60) - 1  # below r: canonical
        m[d:] = 0
        lib.fr_ntt_columns_device(m.data_ptr(), rows, width, "fft")
        first = m.clone()
        halves = random_halves(rows, sets, 1)
        work = torch.empty_like(m)  # what the four transforms run over
        work.copy_(m)
        dev_call, dev_ntt = [], []

        def recover(halves=halves, m=m, rows=rows, width=width, d=d):
            rep, _ = lib.fr_recover_columns_device(halves, m.data_ptr(), rows, width, d, want_first_bad=False)
            dev_call.append(lib.last_timing()[:2])
            if rep["consistent"] != 1:
                sys.exit("rows %d width %d sets %d: not consistent" % (rows, width, sets))

        def four_transforms(work=work, total=total):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for kind in ("ifft", "fft", "ifft", "fft"):
                lib.ntt_device_batch(work.data_ptr(), total // 64, 64, kind)
            e1.record()
            e1.synchronize()
            dev_ntt.append(e0.elapsed_time(e1))
        lib.set_timing(1)
        ta, tb = pairs(args.pairs, recover, four_transforms)
        lib.set_timing(0)
        torch.cuda.synchronize()
        if not torch.equal(m, first):
            sys.exit("rows %d width %d sets %d: a recovery is wrong" % (rows, width, sets))
        dev_call, dev_ntt = dev_call[1:], dev_ntt[1:]  # the warm pair
        t0, t1 = float(np.median([t[0] for t in dev_call])), float(np.median([t[1] for t in dev_call]))
        lg = rows.bit_length() - 1
        products = (4 * lg // 2 + 4) * total
        model = products / GMULS * 1e3
        say("rows %4d width %6d sets %4d, half the rows of every set missing, d = rows / 2  %s  %s; device ms: vanishing values + tables %.3f, decode kernel "
            "%.3f (min %.3f max %.3f); (a) %d products = %.3f ms at 150 Gmul/s: the decode kernel is %.2f times that; (b) four ntt_device_batch calls of 64 x "
            "2^%d: %.3f ms of device time (min %.3f max %.3f): the decode kernel is %.2f times that"
            % (rows, width, sets, show("fr_recover_columns_device", ta), show("4 x ntt_device_batch", tb), t0, t1, min(t[1] for t in dev_call),
               max(t[1] for t in dev_call), products, model, t1 / model, (total // 64).bit_length() - 1, float(np.median(dev_ntt)), min(dev_ntt), max(dev_ntt),
               t1 / float(np.median(dev_ntt))))
        del m, first, work
        torch.cuda.empty_cache()
    say("# NOT timed: the host twin; bbgpu_fr_ntt_columns_device on its own; rows >= 1024 against a wider tile (two passes), whose row segments would fill "
        "a 128-byte line; widths that are not a multiple of the tile's columns; sets that miss different numbers of rows in one call; a call with "
        "first_bad_out (one more read-back of width x 4 bytes); any shape on a non-default stream")
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
