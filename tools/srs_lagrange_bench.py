"""What bbgpu_srs_lagrange costs on one MI355X (profiles/srs_lagrange.txt is this tool's output): per size, wall milliseconds (median / min of `--reps`
calls after two warm ones; the new handle is released outside the timed region) of
  convert        bbgpu_srs_lagrange of a generated table, resident only
  +host_table    the same with the 2n-entry host table exported and read back
  no_tables      resident only with bbgpu_set_precompute(0): the call without the window tables of the new handle
  stages / load / finish   the device time of the log2 n stage launches, of k_lagrange_load and of k_lagrange_finish, from the events bbgpu_set_timing(1)
                 puts between them (median / min over the same calls)
  ns/butterfly   stage time over the butterflies that run a ladder, n/2 log2 n - (n - 1) of them (the twiddle of the others is 1), and over all of them
  update ns/row  k_srs_update alone over the same n rows IN THE SAME RUN: the yardstick -- a butterfly is that ladder without the inversion, with two
                 additions and the common denominators of its table, so ns/butterfly should stay within 10 % of it (boxes differ by +- 5 % on one binary)
  Gmul/s         laddered butterflies x field products per butterfly / stage time; the products are counted from csrc/g1_ladder.hpp (below)
and the host twin bbgpu_host_srs_lagrange at 2^12 rows for scale.  Usage: python tools/srs_lagrange_bench.py [--sizes 4096,65536,1048576] [--reps 5]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.srs_update_bench import products_per_row  # noqa: E402


def products_per_butterfly(n, wb=3):
    """field products one lane of k_lagrange_stage issues for a butterfly with a ladder, averaged over the stages of a size-n conversion: a doubling is 9
    (dbl_pt: mul_sub counts two), an addition 14 (add_pt), the addition into an accumulator at infinity 1"""
    lg = n.bit_length() - 1
    windows, nt = (129 + wb - 1) // wb, 1 << (wb - 1)
    exps = [pos * (n >> (s + 1)) for s in range(lg) for pos in range(1, 1 << s)]  # the exponent of omega^-1, once per (stage, position)
    weights = [n >> (s + 1) for s in range(lg) for pos in range(1, 1 << s)]        # butterflies that share it
    power = sum(w * (e.bit_length() + bin(e).count("1")) for e, w in zip(exps, weights)) / max(1, sum(weights))
    fixed = 1 + 1                                        # w -> plain integer; lambda |t| of the split
    table = 9 + 14 * (nt - 1) + (6 * nt - 10) + 2 * nt  # 2 P, the odd multiples, the factors of the common denominators, applying them
    ladder = 9 * wb * (windows - 1) + 14 * (2 * windows - 1) + 1 + windows  # doublings, additions, the first addition, beta x per window
    skews = 2 * 14 + 1                                   # a wave takes both whenever one lane needs them
    butterfly = 2 * 14                                   # a + t, a - t
    return power + fixed + table + ladder + skews + butterfly


def timed(fn, reps, after):
    """wall ms of fn() and what `after(result)` returns for each timed call (outside the timed region)"""
    for _ in range(2):
        after(fn())
    ts, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
        extra.append(after(r))
    return (statistics.median(ts), min(ts)), extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=4096)
    args = ap.parse_args()
    from barretenberg_amd import BbGpu
    G = BbGpu(device=0)
    rng = np.random.default_rng(7)

    def scalar():
        return np.array([rng.integers(0, 1 << 63, dtype=np.uint64) for _ in range(3)] + [np.uint64(rng.integers(0, 1 << 59))], dtype=np.uint64)
    x, y = scalar(), scalar()
    print("# %s; wall ms, median / min of %d; 3-bit windows" % (G.version(), args.reps))
    m = args.host_rows
    hm, tm = G.srs_generate(x, m, want_host_table=True)
    new, table, _ = G.srs_lagrange(hm, m, want_host_table=True)
    G.srs_release(new)
    host_table, _ = G.host_srs_lagrange(tm, m)
    assert np.array_equal(table, host_table), "the GPU table and the host twin's differ"
    G.srs_release(hm)
    G.set_timing(1)

    def release(r):
        G.srs_release(r[0])
        return G.last_timing()[:3]
    for n in [int(s) for s in args.sizes.split(",")]:
        lg = n.bit_length() - 1
        h = G.srs_generate(x, n)
        conv, k1 = timed(lambda: G.srs_lagrange(h, n), args.reps, release)
        tab, k2 = timed(lambda: G.srs_lagrange(h, n, want_host_table=True), args.reps, release)
        G.set_precompute(False)
        bare, k3 = timed(lambda: G.srs_lagrange(h, n), args.reps, release)
        _, upd = timed(lambda: G.srs_update(h, n, y), args.reps, lambda r: (G.srs_release(r[0]), G.last_timing()[0])[1])
        G.set_precompute(True)
        ks = k1 + k2 + k3
        stage, load, fin = ([k[i] for k in ks] for i in range(3))
        sm, smin = statistics.median(stage), min(stage)
        laddered, every = n // 2 * lg - (n - 1), n // 2 * lg
        um = statistics.median(upd)
        ppb, ppr = products_per_butterfly(n), products_per_row(n)
        print("n %8d  convert %9.3f / %9.3f  +host_table %9.3f / %9.3f  no_tables %9.3f / %9.3f  stages %9.3f / %9.3f  load %8.3f  finish %8.3f" %
              (n, conv[0], conv[1], tab[0], tab[1], bare[0], bare[1], sm, smin, statistics.median(load), statistics.median(fin)))
        print("            ns/butterfly %7.2f with a ladder (%d), %7.2f over all (%d)  products/butterfly %7.1f  Gmul/s %6.1f" %
              (sm * 1e6 / max(1, laddered), laddered, sm * 1e6 / every, every, ppb, laddered * ppb / (sm * 1e-3) / 1e9))
        print("            k_srs_update, same run: %9.3f / %9.3f ms  ns/row %7.2f  products/row %7.1f  Gmul/s %6.1f  ->  butterfly / row = %.3f" %
              (um, min(upd), um * 1e6 / n, ppr, n * ppr / (um * 1e-3) / 1e9, (sm / max(1, laddered)) / (um / n)))
        G.srs_release(h)
    G.set_timing(0)
    host = timed(lambda: G.host_srs_lagrange(tm, m), 3, lambda r: None)[0]
    print("host twin  n %8d  %9.3f / %9.3f ms  (%d threads at most)" % (m, host[0], host[1], min(16, os.cpu_count() or 1)))
    G.shutdown()


if __name__ == "__main__":
    main()
