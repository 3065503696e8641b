"""What bbgpu_kzg_check_open_cosets costs (profiles/kzg_check_cells.txt is this tool's output, below the kernels' resource lines handed over through
--head): one process on one MI355X, every leg warm.  Wall milliseconds per CALL around the C entry, Python binding included; every call ends synchronised
(it returns the verdict).  Cells: `batch` polynomials of n random coefficients over a generated string, committed to (bbgpu_msm_g1_device), transformed
(bbgpu_ntt_device_batch) and opened on every coset of l points (bbgpu_kzg_open_cosets_device) by the device; fixed seed, no LOCATE; every report is checked
to say ok.
  wall        bbgpu_kzg_check_open_cosets(n, l, batch): batch x n values and batch x n / l proofs cross the link
  stages      bbgpu_kzg_check_last_timing: uploads + k_kzg_cells + k_kzg_cell_coefficients + the findings' read-back | the fold | the two MSMs | the host
              tail (two normalisations and the pairing check); medians over the same calls
  kernel      k_kzg_cell_coefficients alone from device events (bbgpu_set_timing, calls of their own: the events add a synchronisation), beside the count
              of field products per value, 2 log2 n + log2 l + 3, at the 150 Gmul/s measured for fe_mont_gfx950.h (an estimate of the arithmetic alone)
  bar         bbgpu_kzg_check_open_cosets at --bar n,l,batch against bbgpu_kzg_check_open_all at the same n and batch over the SAME values (its proofs by
              bbgpu_kzg_open_all_device), in this process, in alternating pairs: medians, full ranges, and whether the new entry's median exceeds the old
              one's by more than the larger range
Usage: python tools/kzg_check_cells_bench.py [--reps 9] [--sizes 4096:64:1,65536:64:1,65536:64:16,65536:4:1,1048576:64:1] [--bar 65536:64:16] [--head FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = np.arange(1, 5, dtype=np.uint64)
STAGES = ("claims_ms", "fold_ms", "msm_ms", "host_tail_ms")
GMULS = 150e9  # field products per second measured for fe_mont_gfx950.h (profiles/README.md)


def show(ts):
    q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
    return "%9.3f (min %9.3f max %9.3f iqr %7.3f)" % (statistics.median(ts), min(ts), max(ts), q[2] - q[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="4096:64:1,65536:64:1,65536:64:16,65536:4:1,1048576:64:1")
    ap.add_argument("--bar", default="65536:64:16")
    ap.add_argument("--head", default=None)
    args = ap.parse_args()
    import pathlib
    import tempfile

    import torch
    from barretenberg_amd import BbGpu
    from oracle.pyoracle import Oracle, aligned_copy, build
    from tests.kzg_check_cells_cases import g2_of, power_of_secret, secret_x
    build()
    oracle, lib = Oracle(), BbGpu(device=0)
    if args.head:
        sys.stdout.write(open(args.head).read())
    sizes = [tuple(int(v) for v in s.split(":")) for s in args.sizes.split(",") if s]
    bar = tuple(int(v) for v in args.bar.split(":")) if args.bar else None
    x = secret_x(oracle)
    tmp = pathlib.Path(tempfile.mkdtemp())
    g2_x = g2_of(lib, oracle, tmp, x, "x.dat")
    g2_xl = {l: g2_of(lib, oracle, tmp, power_of_secret(oracle, l), "x%d.dat" % l) for l in {s[1] for s in sizes + ([bar] if bar else [])}}
    h64, table = lib.srs_generate(x, 64, want_host_table=True)
    lib.srs_release(h64)
    h = lib.srs_generate(x, max(s[0] for s in sizes + ([bar] if bar else [])))
    print("# %s; wall ms per CALL: median (min, max, interquartile range) of %d calls after two warm ones" % (lib.version(), args.reps))

    def world(n, l, batch, singles=False):
        c = aligned_copy(oracle.random_scalars(0xBE7C + n + l, batch * n))
        d_c = torch.from_numpy(c.view(np.int64)).cuda()
        setup = lib.kzg_open_cosets_setup(h, n, l)
        proofs = lib.kzg_open_cosets_device(setup, d_c.data_ptr(), n, l, batch=batch)
        lib.kzg_open_cosets_release(setup)
        single = None
        if singles:
            setup = lib.kzg_open_all_setup(h, n)
            single = lib.kzg_open_all_device(setup, d_c.data_ptr(), n, batch=batch)
            lib.kzg_open_all_release(setup)
        d_y = d_c.clone()
        torch.cuda.synchronize()
        commitments = np.stack([lib.msm_device(h, d_c.data_ptr() + b * n * 32, n)[:8] for b in range(batch)])
        lib.ntt_device_batch(d_y.data_ptr(), n, batch, "fft")
        torch.cuda.synchronize()
        values = d_y.cpu().numpy().view(np.uint64).reshape(batch * n, 4).copy()
        del d_c, d_y
        return commitments, values, proofs, single, aligned_copy(table[0:2 * l:2])

    def timed(call):
        t0 = time.perf_counter()
        rep = call()
        t1 = time.perf_counter()
        assert rep["ok"] == 1, rep
        return (t1 - t0) * 1e3

    for n, l, batch in sizes:
        commitments, values, proofs, _, head = world(n, l, batch)
        call = lambda: lib.kzg_check_open_cosets(commitments, values, proofs, n, l, head, g2_xl[l], batch=batch, seed=SEED)  # noqa: E731
        total, stages = [], {k: [] for k in STAGES}
        for k in range(args.reps + 2):
            ms = timed(call)
            if k >= 2:
                total.append(ms)
                st = lib.kzg_check_last_timing()
                for s in STAGES:
                    stages[s].append(st[s])
        st = {s: statistics.median(v) for s, v in stages.items()}
        lib.set_timing(True)
        kernel = []
        for k in range(args.reps + 1):
            timed(call)
            if k:
                kernel.append(lib.last_timing()[0])
        lib.set_timing(False)
        products = 2 * (n.bit_length() - 1) + (l.bit_length() - 1) + 3
        print("n %8d  l %2d  batch %2d  cells %6d  %s   upload + cell kernels %8.3f  fold %6.3f  msms %8.3f  host tail %6.3f" %
              (n, l, batch, batch * n // l, show(total), st["claims_ms"], st["fold_ms"], st["msm_ms"], st["host_tail_ms"]), flush=True)
        print("    k_kzg_cell_coefficients from events, ms: %s; %d values x %d products = %.3f ms at 150 Gmul/s (an estimate of the arithmetic alone)" %
              (show(kernel), batch * n, products, batch * n * products / GMULS * 1e3), flush=True)
    if bar:
        n, l, batch = bar
        commitments, values, proofs, single, head = world(n, l, batch, singles=True)
        new = lambda: lib.kzg_check_open_cosets(commitments, values, proofs, n, l, head, g2_xl[l], batch=batch, seed=SEED)  # noqa: E731
        old = lambda: lib.kzg_check_open_all(commitments, values, single, n, g2_x, batch=batch, seed=SEED)  # noqa: E731
        for k in range(2):
            timed(new), timed(old)
        t_new, t_old = [], []
        for k in range(args.reps):
            t_new.append(timed(new))
            t_old.append(timed(old))
        margin = max(max(t_new) - min(t_new), max(t_old) - min(t_old))
        m_new, m_old = statistics.median(t_new), statistics.median(t_old)
        print("bar at n %d, l %d, batch %d (%d values), %d alternating pairs:" % (n, l, batch, batch * n, args.reps))
        print("    bbgpu_kzg_check_open_cosets  %s" % show(t_new))
        print("    bbgpu_kzg_check_open_all     %s" % show(t_old))
        print("    new - old = %+.3f ms, margin (the larger full range) %.3f ms: the bar is %s" %
              (m_new - m_old, margin, "MET" if m_new <= m_old else ("met within the margin" if m_new - m_old <= margin else "MISSED")), flush=True)
    print("staging after the run: %d bytes" % lib.memory_stats()["staging_bytes"])
    lib.srs_release(h)
    lib.shutdown()


if __name__ == "__main__":
    main()
