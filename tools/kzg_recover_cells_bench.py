"""What bbgpu_kzg_recover_cells costs -- `batch` polynomials rebuilt from the same subset of their cells -- and where the time goes
(profiles/kzg_recover_cells.txt is this tool's output): one process on one MI355X, every leg warm, the two legs of a shape alternating inside every pair (the
order swapped from pair to pair), medians of --pairs pairs.  Wall milliseconds per call around the C entries, Python binding included, each leg ended by a
device synchronise; the legacy default stream.  The polynomials are honest: random coefficients below the degree bound n / 2 on the device, their values by
bbgpu_ntt_device_batch, the listed cells gathered on the host, so that the tail issues no atomic.
  recover     one bbgpu_kzg_recover_cells call with the transforms read back (values_out given): the values cross to the device, the coefficients stay
              there, batch x n x 32 bytes come back.
  transforms  the same four bbgpu_ntt_device_batch calls alone (IFFT, COSET_FFT, COSET_IFFT in place, FFT on a second buffer), nothing crossing the link.
The difference of the two is what the vanishing values, the batch inversion, scatter, divide, tail and the copies cost.
(n, l, batch) = (8192, 64, 1), (8192, 64, 64), (2^16, 64, 16), (2^20, 64, 1), (2^20, 64, 4), each with every other cell missing and with one cell missing.
The device times of one call per shape come from bbgpu_set_timing.  k_recover_vanish is held against its own product count, 2 mu m, at the 150 G products
per second measured for the product of csrc/fe_mont_gfx950.h (150.3 Gmul/s, profiles/r02_ubench_mul.txt; an estimate of the arithmetic alone): the line prints the count, the time that
rate would take and the ratio measured / that time.  No ratio is asserted.
Caveat (profiles/r05_ntt_ramp.txt): after an idle spell the device clock takes some 30 ms of work to come up, and the first transforms of a burst run up to a
quarter slower; a leg here is preceded by the other leg and by a warm pair, but the legs of the small shapes are shorter than the ramp, so their medians
carry some of it -- both legs alike.
--head FILE puts the lines of FILE in front of the output (the compiler's resource remarks for csrc/kzg_recover_cells.hip, which no run on the GPU can make).
Usage: python tools/kzg_recover_cells_bench.py [--pairs 9] [--head FILE] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.lagrange_open_bench import LINES, pairs, say, show, stats  # noqa: E402  (the same clock, pairing and report lines)

PRODUCTS_PER_SECOND = 150e9
SHAPES = ((13, 64, 1), (13, 64, 64), (16, 64, 16), (20, 64, 1), (20, 64, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_recover_cells.txt"))
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
    say("# recover: bbgpu_kzg_recover_cells with values_out; transforms: IFFT, COSET_FFT, COSET_IFFT and FFT by bbgpu_ntt_device_batch alone, no copy")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x2EC0)
    for lg, l, batch in SHAPES:
        n = 1 << lg
        m, d = n // l, n // 2
        c = torch.randint(-(1 << 63), (1 << 63) - 1, (batch, n, 4), dtype=torch.int64, device="cuda", generator=gen)
        c[:, d:] = 0
        v = c.clone()
        lib.ntt_device_batch(v.data_ptr(), n, batch, "fft")
        torch.cuda.synchronize()
        values_all = v.cpu().numpy().view(np.uint64).reshape(batch, l, m, 4)  # element k + m j of polynomial b at [b, j, k]
        want = v.cpu().numpy().view(np.uint64).reshape(batch, n, 4)
        lib.ntt_device_batch(v.data_ptr(), n, batch, "ifft")  # the coefficients again, canonical
        torch.cuda.synchronize()
        want_c = v.cpu().numpy().view(np.uint64)
        d_out, d_second = torch.zeros_like(c), torch.zeros_like(c)
        h_out = np.zeros((batch, n, 4), dtype=np.uint64)  # values_out: the caller's buffer, made once as a caller would
        for name, missing in (("every other cell missing", list(range(0, m, 2))), ("one cell missing", [m // 3])):
            gone = set(missing)
            cells = np.array([k for k in range(m) if k not in gone], dtype=np.uint32)
            values = np.ascontiguousarray(values_all[:, :, cells].transpose(0, 2, 1, 3)).reshape(-1, 4)
            mu = len(missing)

            def recover():
                return lib.kzg_recover_cells(cells, values, n, l, d, d_out.data_ptr(), batch=batch, out=h_out)

            def transforms():
                for kind in ("ifft", "coset_fft", "coset_ifft"):
                    lib.ntt_device_batch(d_out.data_ptr(), n, batch, kind)
                lib.ntt_device_batch(d_second.data_ptr(), n, batch, "fft")
            got, rep = recover()
            torch.cuda.synchronize()
            if not (np.array_equal(got, want) and rep["consistent"] == 1 and np.array_equal(d_out.cpu().numpy().view(np.uint64), want_c)):
                sys.exit("n 2^%d l %d batch %d, %s: the recovery is wrong" % (lg, l, batch, name))
            ta, tb = pairs(args.pairs, recover, transforms)
            sa, sb = stats(ta), stats(tb)
            say("n 2^%d l %2d batch %2d, %s (mu %d of %d)  %s  %s  recover - transforms: %.3f ms of medians (full ranges %.3f and %.3f)"
                % (lg, l, batch, name, mu, m, show("recover", ta), show("transforms", tb), sa["med"] - sb["med"], sa["hi"] - sa["lo"], sb["hi"] - sb["lo"]))
            lib.set_timing(1)
            recover()
            ms = lib.last_timing()
            lib.set_timing(0)
            products = 2 * mu * m
            ideal = products / PRODUCTS_PER_SECOND * 1e3
            say("n 2^%d l %2d batch %2d, %s  device ms: k_recover_vanish %.4f, scatter + IFFT %.3f, coset FFT + divide + coset IFFT + tail %.3f, FFT %.3f; "
                "k_recover_vanish: %d products, %.4f ms at 150 G/s, measured / that = %.2f"
                % ((lg, l, batch, name) + tuple(ms) + (products, ideal, ms[0] / ideal)))
        del c, v, d_out, d_second
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
