"""What bbgpu_srs_update costs on one MI355X (profiles/srs_update.txt is this tool's output): per size, wall milliseconds (median / min of `--reps` calls
after two warm ones; the new handle is released outside the timed region) of
  update         bbgpu_srs_update of a generated table, y random, x * G2 given, resident only
  +host_table    the same with the 2n-entry host table exported and read back
  no_tables      resident only with bbgpu_set_precompute(0): the call without the window tables of the new handle
  kernel         k_srs_update alone, from the pair of events bbgpu_set_timing(1) puts around it (median / min over the same calls)
  Gmul/s         rows x field products per row / kernel time; the products are counted from csrc/srs_update.hip (products_per_row below), against the
                 150 Gmul/s of the multiplier alone (README)
and the host twin bbgpu_host_srs_update at 2^12 rows for scale.  Usage: python tools/srs_update_bench.py [--sizes 65536,1048576] [--reps 7]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FQ_MODULUS = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def products_per_row(n, first=0, wb=3):
    """field products one lane of k_srs_update<wb> issues, averaged over rows [first, first + n): a doubling is 9 (dbl_pt: mul_sub counts two), an addition
    14 (add_pt), the addition into an accumulator at infinity 1"""
    windows = (129 + wb - 1) // wb
    power = sum(e.bit_length() + bin(e).count("1") for e in range(first, first + n)) / n  # square-and-multiply on the exponent, Fr
    fixed = 1 + 1                                        # s -> plain integer; lambda |t| of the split
    table = 9 + 14 * ((1 << (wb - 1)) - 1)              # 2 P, then the odd multiples
    ladder = 9 * wb * (windows - 1) + 14 * (2 * windows - 1) + 1 + windows  # doublings, additions, the first addition, beta x per window
    skews = 2 * 14 + 1                                   # a wave takes both whenever one lane needs them
    inverse = 256 + bin(FQ_MODULUS - 2).count("1") + 5  # Fermat chain, then zz zzz, the two inverses, x, y
    return power + fixed + table + ladder + skews + inverse


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
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=4096)
    args = ap.parse_args()
    from barretenberg_amd import BbGpu
    G = BbGpu(device=0)
    rng = np.random.default_rng(7)

    def scalar():
        return np.array([rng.integers(0, 1 << 63, dtype=np.uint64) for _ in range(3)] + [np.uint64(rng.integers(0, 1 << 59))], dtype=np.uint64)
    x, y = scalar(), scalar()
    fd, tiny_path = tempfile.mkstemp(suffix=".dat")
    os.close(fd)
    h2, tiny = G.srs_generate(x, 2, want_host_table=True)
    G.srs_release(h2)
    G.write_transcript(tiny_path, tiny, 2, x)
    g2_x = G.transcript_read_g2(tiny_path)
    os.unlink(tiny_path)
    wb = 3  # SRS_UPDATE_WB of csrc/srs_update.hip, for the product count
    print("# %s; wall ms, median / min of %d; %d-bit windows" % (G.version(), args.reps, wb))
    G.set_timing(1)

    def release(r):
        G.srs_release(r[0])
        return G.last_timing()[0]
    for n in [int(s) for s in args.sizes.split(",")]:
        h = G.srs_generate(x, n)
        new, table, rep = G.srs_update(h, n, y, g2_x, want_host_table=True)
        assert G.srs_check(new, n, np.array(rep.g2_x_out, dtype=np.uint64)).ok and G.host_srs_update_check(tiny[2], table[2], np.array(rep.y_g2, dtype=np.uint64))
        G.srs_release(new)
        upd, kernel = timed(lambda: G.srs_update(h, n, y, g2_x), args.reps, release)
        tab, _ = timed(lambda: G.srs_update(h, n, y, g2_x, want_host_table=True), args.reps, release)
        G.set_precompute(False)
        bare, kernel2 = timed(lambda: G.srs_update(h, n, y, g2_x), args.reps, release)
        G.set_precompute(True)
        g2 = timed(lambda: G.host_srs_update(tiny, 1, y, g2_x), args.reps, lambda r: None)[0]
        ks = kernel + kernel2
        km, kmin = statistics.median(ks), min(ks)
        ppr = products_per_row(n, 0, wb)
        print("n %8d  update %9.3f / %9.3f  +host_table %9.3f / %9.3f  no_tables %9.3f / %9.3f  kernel %9.3f / %9.3f  products/row %7.1f  Gmul/s %6.1f  "
              "(G2 half + one host row %6.3f / %6.3f)" % (n, upd[0], upd[1], tab[0], tab[1], bare[0], bare[1], km, kmin, ppr, n * ppr / (km * 1e-3) / 1e9, g2[0], g2[1]))
        G.srs_release(h)
    G.set_timing(0)
    m = args.host_rows
    hm, tm = G.srs_generate(x, m, want_host_table=True)
    G.srs_release(hm)
    host = timed(lambda: G.host_srs_update(tm, m, y, g2_x), max(3, args.reps // 2), lambda r: None)[0]
    print("host twin  n %8d  %9.3f / %9.3f ms  (%d threads at most)" % (m, host[0], host[1], min(16, os.cpu_count() or 1)))
    G.shutdown()


if __name__ == "__main__":
    main()
