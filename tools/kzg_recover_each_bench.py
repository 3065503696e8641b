"""What bbgpu_kzg_recover_cells_each costs -- polynomials rebuilt from cell sets of their own, the vanishing polynomials from a product tree -- beside
bbgpu_kzg_recover_cells (profiles/kzg_recover_each.txt is this tool's output): one process on one MI355X, every leg warm, the two legs of a line alternating
inside every pair (the order swapped from pair to pair), medians of --pairs pairs.  Wall milliseconds per call around the C entries, Python binding
included, each leg ended by a device synchronise; the legacy default stream; values_out read back into a buffer made once.  The polynomials are honest:
random coefficients below the degree bound n / 2 on the device, their values by bbgpu_ntt_device_batch, the listed cells gathered on the host.
  same   every polynomial holds the same cells: `each` (the new entry) beside `cells` (bbgpu_kzg_recover_cells), at (n, l, batch) = (8192, 64, 1),
         (2^16, 64, 16), (2^20, 64, 1), (2^20, 64, 4), every other cell missing and one cell missing.
  differ every polynomial misses its own random half of the cells: ONE call of the new entry beside `batch` calls of bbgpu_kzg_recover_cells at batch 1,
         at (2^16, 64, 16) and (2^20, 64, 4).
  new    the shapes only the new entry takes, (2^20, 1, 1) and (2^20, 4, 4), a random half of the cells missing, beside the four transforms alone.
The device times of one call per line come from bbgpu_set_timing: the tree (leaves, levels, gather and the two Z transforms), scatter + IFFT, coset FFT +
divide + coset IFFT + tail, FFT.  The leaves' own product count, M T per polynomial, and the time the 150 G products per second of csrc/fe_mont_gfx950.h
would take for it are printed beside; the kernel's own time is not in bbgpu_last_timing (a kernel trace gives it).  No ratio is asserted.
--head FILE puts the lines of FILE in front of the output.  --only KIND[,KIND] runs some of same, differ, new.  --leaf T states the leaf size of a
comparison build named by BBGPU_LIB (KZG_RECOVER_EACH_LEAF = 256 in csrc/bbgpu_internal.h, built with make -C barretenberg_amd/csrc variant NAME=leaf256).
Usage: python tools/kzg_recover_each_bench.py [--pairs 9] [--only same,differ,new] [--leaf T] [--head FILE] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.lagrange_open_bench import LINES, line, pairs, say, show  # noqa: E402  (the same clock, pairing and report lines)

PRODUCTS_PER_SECOND = 150e9
SAME = ((13, 64, 1), (16, 64, 16), (20, 64, 1), (20, 64, 4))
DIFFER = ((16, 64, 16), (20, 64, 4))
NEW = ((20, 1, 1), (20, 4, 4))


def world(lib, gen, lg, l, batch):
    import torch
    n = 1 << lg
    c = torch.randint(-(1 << 63), (1 << 63) - 1, (batch, n, 4), dtype=torch.int64, device="cuda", generator=gen)
    c[:, n // 2:] = 0
    v = c.clone()
    lib.ntt_device_batch(v.data_ptr(), n, batch, "fft")
    torch.cuda.synchronize()
    values = v.cpu().numpy().view(np.uint64).reshape(batch, n, 4).copy()
    lib.ntt_device_batch(v.data_ptr(), n, batch, "ifft")  # the coefficients again, canonical
    torch.cuda.synchronize()
    return values, v.cpu().numpy().view(np.uint64).reshape(batch, n, 4).copy()


def gather(values, l, cells):
    """(count, l, 4) of one polynomial's (n, 4) values"""
    return np.ascontiguousarray(values.reshape(l, -1, 4)[:, cells].transpose(1, 0, 2))


LEAF = [None]  # --leaf: the T of the library under test when it is not the shipped one (BBGPU_LIB names a comparison build)


def device_times(lib, call, lg, l, batch, what, max_mu):
    from barretenberg_amd import BbGpu
    lib.set_timing(1)
    call()
    ms = lib.last_timing()
    lib.set_timing(0)
    T, M = LEAF[0] or BbGpu.RECOVER_EACH_LEAF, 1
    while M < max_mu:
        M <<= 1
    products = batch * M * min(T, M)
    say("n 2^%d l %2d batch %2d, %s  device ms: tree + Z transforms %.4f, scatter + IFFT %.3f, coset FFT + divide + coset IFFT + tail %.3f, FFT %.3f; "
        "leaves: T %d, M %d, %d products, %.4f ms at 150 G/s"
        % ((lg, l, batch, what) + tuple(ms) + (min(T, M), M, products, products / PRODUCTS_PER_SECOND * 1e3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--only", default="same,differ,new")
    ap.add_argument("--leaf", type=int, default=None)
    ap.add_argument("--head", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_recover_each.txt"))
    args = ap.parse_args()
    LEAF[0] = args.leaf
    import torch
    from barretenberg_amd import BbGpu
    if args.head:
        with open(args.head) as fh:
            for text in fh.read().splitlines():
                say(text)
    lib = BbGpu(device=0)
    say("# %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of %d alternating pairs after a warm pair" %
        (lib.version(), args.pairs))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x2EC3)
    rng = np.random.default_rng(0x2EC3)
    only = args.only.split(",")

    def check(got, rep, d_out, values, coeffs, what):
        torch.cuda.synchronize()
        if not (np.array_equal(got, values) and rep["consistent"] == 1 and np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(coeffs.shape), coeffs)):
            sys.exit("%s: the recovery is wrong" % what)

    for lg, l, batch in SAME if "same" in only else ():
        n = 1 << lg
        m, d = n // l, n // 2
        values, coeffs = world(lib, gen, lg, l, batch)
        d_out = torch.zeros((batch, n, 4), dtype=torch.int64, device="cuda")
        h_out = np.zeros((batch, n, 4), dtype=np.uint64)
        for name, missing in (("every other cell missing", np.arange(0, m, 2)), ("one cell missing", np.array([m // 3]))):
            cells = np.setdiff1d(np.arange(m), missing).astype(np.uint32)
            per = [gather(values[b], l, cells) for b in range(batch)]
            flat = np.ascontiguousarray(np.concatenate(per).reshape(-1, 4))
            each = lambda: lib.kzg_recover_cells_each([cells] * batch, flat, n, l, d, d_out.data_ptr(), out=h_out)  # noqa: E731
            old = lambda: lib.kzg_recover_cells(cells, flat, n, l, d, d_out.data_ptr(), batch=batch, out=h_out)  # noqa: E731
            what = "same sets, n 2^%d l %2d batch %2d, %s (mu %d of %d)" % (lg, l, batch, name, len(missing), m)
            got, rep, _ = each()
            check(got, rep, d_out, values, coeffs, what)
            ta, tb = pairs(args.pairs, each, old)
            line(what, "each", ta, "cells", tb)
            device_times(lib, each, lg, l, batch, name, len(missing))
        del d_out

    for lg, l, batch in DIFFER if "differ" in only else ():
        n = 1 << lg
        m, d = n // l, n // 2
        values, coeffs = world(lib, gen, lg, l, batch)
        d_out = torch.zeros((batch, n, 4), dtype=torch.int64, device="cuda")
        h_out = np.zeros((batch, n, 4), dtype=np.uint64)
        cells = [np.ascontiguousarray(rng.permutation(m)[:m // 2].astype(np.uint32)) for _ in range(batch)]
        per = [gather(values[b], l, c) for b, c in enumerate(cells)]
        flats = [np.ascontiguousarray(p.reshape(-1, 4)) for p in per]
        whole = np.ascontiguousarray(np.concatenate(flats))
        each = lambda: lib.kzg_recover_cells_each(cells, whole, n, l, d, d_out.data_ptr(), out=h_out)  # noqa: E731

        def one_by_one():
            for b in range(batch):
                lib.kzg_recover_cells(cells[b], flats[b], n, l, d, d_out.data_ptr() + 32 * n * b, batch=1, out=h_out[b:b + 1])
        what = "different sets, n 2^%d l %2d batch %2d, a random half of the cells missing" % (lg, l, batch)
        got, rep, _ = each()
        check(got, rep, d_out, values, coeffs, what)
        ta, tb = pairs(args.pairs, each, one_by_one)
        line(what, "each, one call", ta, "cells, %d calls" % batch, tb)
        device_times(lib, each, lg, l, batch, "different sets", m - m // 2)
        del d_out

    for lg, l, batch in NEW if "new" in only else ():
        n = 1 << lg
        m, d = n // l, n // 2
        values, coeffs = world(lib, gen, lg, l, batch)
        d_out = torch.zeros((batch, n, 4), dtype=torch.int64, device="cuda")
        d_second = torch.zeros((batch, n, 4), dtype=torch.int64, device="cuda")
        h_out = np.zeros((batch, n, 4), dtype=np.uint64)
        cells = [np.ascontiguousarray(rng.permutation(m)[:m // 2].astype(np.uint32)) for _ in range(batch)]
        per = [gather(values[b], l, c) for b, c in enumerate(cells)]
        whole = np.ascontiguousarray(np.concatenate(per).reshape(-1, 4))
        each = lambda: lib.kzg_recover_cells_each(cells, whole, n, l, d, d_out.data_ptr(), out=h_out)  # noqa: E731

        def transforms():
            for kind in ("ifft", "coset_fft", "coset_ifft"):
                lib.ntt_device_batch(d_out.data_ptr(), n, batch, kind)
            lib.ntt_device_batch(d_second.data_ptr(), n, batch, "fft")
        what = "new shapes, n 2^%d l %2d batch %2d, a random half of the cells missing" % (lg, l, batch)
        got, rep, _ = each()
        check(got, rep, d_out, values, coeffs, what)
        ta, tb = pairs(args.pairs, each, transforms)
        say("%s  %s  %s" % (what, show("each", ta), show("transforms", tb)))
        device_times(lib, each, lg, l, batch, "different sets", m - m // 2)
        del d_out, d_second
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
