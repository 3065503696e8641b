"""What the layout entries of the check of KZG cell proofs cost beside the entries of 64 commitments (profiles/kzg_check_layout.txt is this tool's output;
run by hand, not by bench.py): one process on one MI355X, every leg warm.  Wall milliseconds per CALL around the C entry, Python binding included; every
call ends synchronised (it returns the verdict).  Medians of --reps calls with the SPREAD of each leg, meaning its full range (max - min).  The data: 64
polynomials of n random coefficients over a generated string, committed to, transformed and opened on every coset of l points by the device; a layout of
`rows` rows takes polynomial c % 64 as row c.  Fixed seed, no LOCATE; every report is checked to say ok.
  eight      (rows, n, l) = (512, 2^11, 64), 2^20 values: ONE bbgpu_kzg_check_open_cosets_layout against EIGHT bbgpu_kzg_check_open_cosets of 64 rows each
             over the same data, in alternating pairs
  same       (64, 2^14, 64): one bbgpu_kzg_check_open_cosets_layout against the one bbgpu_kzg_check_open_cosets it replaces, in alternating pairs; the bar:
             the new entry's median is no higher than the old one's beyond the larger spread of the two legs
  labels     bbgpu_kzg_check_cells_layout over 2^14 cells of 64 values under 512 labels, once with uniform labels and once with every cell on one label,
             in alternating pairs; then, in calls of their own (bbgpu_set_timing: the events add synchronisations), the commitments kernel with the
             grouping and the grouped fold alone from device events.  The bar: the one-label median is within the larger spread of the uniform one
Usage: python tools/kzg_check_layout_bench.py [--reps 9] [--out profiles/kzg_check_layout.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = np.arange(1, 5, dtype=np.uint64)
BASE = 64  # distinct polynomials of a world


def show(ts):
    return "%9.3f (min %9.3f max %9.3f spread %7.3f)" % (statistics.median(ts), min(ts), max(ts), max(ts) - min(ts))


def verdict(m_new, m_old, margin):
    return "MET" if m_new <= m_old else ("met within the spread" if m_new - m_old <= margin else "MISSED")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kzg_check_layout.txt"))
    args = ap.parse_args()
    import pathlib
    import tempfile

    import torch
    from barretenberg_amd import BbGpu
    from oracle.pyoracle import Oracle, aligned_copy, build
    from tests.kzg_check_cells_cases import g2_of, power_of_secret, secret_x
    build()
    oracle, lib = Oracle(), BbGpu(device=0)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    x = secret_x(oracle)
    l = 64
    g2_xl = g2_of(lib, oracle, pathlib.Path(tempfile.mkdtemp()), power_of_secret(oracle, l), "xl.dat")
    h64, table = lib.srs_generate(x, l, want_host_table=True)
    lib.srs_release(h64)
    head = aligned_copy(table[0:2 * l:2])
    h = lib.srs_generate(x, 1 << 14)
    say("# %s; wall ms per CALL: median (min, max, spread = max - min) of %d calls after two warm ones" % (lib.version(), args.reps))

    def world(n):
        """commitments (64, 8), values (64, n, 4), proofs (64, n / l, 8) by the device producers"""
        c = aligned_copy(oracle.random_scalars(0x1A70 + n, BASE * n))
        d_c = torch.from_numpy(c.view(np.int64)).cuda()
        setup = lib.kzg_open_cosets_setup(h, n, l)
        proofs = lib.kzg_open_cosets_device(setup, d_c.data_ptr(), n, l, batch=BASE)
        lib.kzg_open_cosets_release(setup)
        d_y = d_c.clone()
        torch.cuda.synchronize()
        commitments = np.stack([lib.msm_device(h, d_c.data_ptr() + b * n * 32, n)[:8] for b in range(BASE)])
        lib.ntt_device_batch(d_y.data_ptr(), n, BASE, "fft")
        torch.cuda.synchronize()
        return commitments, d_y.cpu().numpy().view(np.uint64).reshape(BASE, n, 4).copy(), np.asarray(proofs).reshape(BASE, n // l, 8)

    def timed(call):
        t0 = time.perf_counter()
        reps = call()
        t1 = time.perf_counter()
        assert all(r["ok"] == 1 for r in (reps if isinstance(reps, list) else [reps])), reps
        return (t1 - t0) * 1e3

    def pairs(a, b):
        for _ in range(2):
            timed(a), timed(b)
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(a))
            tb.append(timed(b))
        return ta, tb

    # ---- eight: 512 rows of 2^11 values
    n, rows = 1 << 11, 512
    commitments, values, proofs = world(n)
    idx = np.arange(rows) % BASE
    cs, vs, ps = aligned_copy(commitments[idx]), aligned_copy(values[idx].reshape(-1, 4)), aligned_copy(proofs[idx].reshape(-1, 8))
    m = n // l
    parts = [(aligned_copy(cs[k:k + 64]), aligned_copy(vs[k * n:(k + 64) * n]), aligned_copy(ps[k * m:(k + 64) * m])) for k in range(0, rows, 64)]
    one = lambda: lib.kzg_check_open_cosets_layout(cs, vs, ps, n, l, head, g2_xl, batch=rows, seed=SEED)  # noqa: E731
    eight = lambda: [lib.kzg_check_open_cosets(c, v, p, n, l, head, g2_xl, batch=64, seed=SEED) for c, v, p in parts]  # noqa: E731
    t_one, t_eight = pairs(one, eight)
    say("eight: (rows, n, l) = (%d, %d, %d), %d values, %d alternating pairs:" % (rows, n, l, rows * n, args.reps))
    say("    one bbgpu_kzg_check_open_cosets_layout      %s" % show(t_one))
    say("    eight bbgpu_kzg_check_open_cosets of 64     %s" % show(t_eight))
    say("    one / eight = %.3f" % (statistics.median(t_one) / statistics.median(t_eight)))

    # ---- labels: 2^14 cells of the same world under 512 labels
    count, S = 1 << 14, 512
    t = np.arange(count)

    def labelled(labels):
        b, k = labels % BASE, (t * 7 + t // BASE) % m
        cell_values = values[b[:, None], k[:, None] + m * np.arange(l)[None, :]].reshape(-1, 4)
        return labels.astype(np.uint32), k.astype(np.uint32), aligned_copy(cell_values), aligned_copy(proofs[b, k])

    forms = {"uniform": labelled(t % S), "one label": labelled(np.full(count, S - 1))}
    call = {name: (lambda a=a: lib.kzg_check_cells_layout(cs, a[0], a[1], a[2], a[3], n, l, head, g2_xl, seed=SEED)) for name, a in forms.items()}
    t_uni, t_single = pairs(call["uniform"], call["one label"])
    margin = max(max(t_uni) - min(t_uni), max(t_single) - min(t_single))
    say("labels: bbgpu_kzg_check_cells_layout, %d cells of %d values under %d labels, %d alternating pairs:" % (count, l, S, args.reps))
    say("    uniform labels                              %s" % show(t_uni))
    say("    every cell on one label                     %s" % show(t_single))
    say("    one label - uniform = %+.3f ms, margin (the larger spread) %.3f ms: within the spread: %s" %
        (statistics.median(t_single) - statistics.median(t_uni), margin, "YES" if abs(statistics.median(t_single) - statistics.median(t_uni)) <= margin else "NO"))
    lib.set_timing(True)
    for name in forms:
        group, fold = [], []
        for k in range(args.reps + 1):
            timed(call[name])
            if k:
                ms = lib.last_timing()
                group.append(ms[1])
                fold.append(ms[2])
        say("    %-10s from device events, ms: commitments + grouping %s" % (name, show(group)))
        say("    %-10s from device events, ms: the grouped fold       %s" % (name, show(fold)))
    lib.set_timing(False)

    # ---- same: 64 rows of 2^14 values
    n, rows = 1 << 14, 64
    commitments, values, proofs = world(n)
    cs, vs, ps = aligned_copy(commitments), aligned_copy(values.reshape(-1, 4)), aligned_copy(proofs.reshape(-1, 8))
    new = lambda: lib.kzg_check_open_cosets_layout(cs, vs, ps, n, l, head, g2_xl, batch=rows, seed=SEED)  # noqa: E731
    old = lambda: lib.kzg_check_open_cosets(cs, vs, ps, n, l, head, g2_xl, batch=rows, seed=SEED)  # noqa: E731
    t_new, t_old = pairs(new, old)
    margin = max(max(t_new) - min(t_new), max(t_old) - min(t_old))
    say("same: (rows, n, l) = (%d, %d, %d), %d values, %d alternating pairs:" % (rows, n, l, rows * n, args.reps))
    say("    bbgpu_kzg_check_open_cosets_layout          %s" % show(t_new))
    say("    bbgpu_kzg_check_open_cosets                 %s" % show(t_old))
    say("    new - old = %+.3f ms, margin (the larger spread) %.3f ms: the bar (no slower at S = 64) is %s" %
        (statistics.median(t_new) - statistics.median(t_old), margin, verdict(statistics.median(t_new), statistics.median(t_old), margin)))
    say("NOT timed: the rounds of LOCATE, more than 512 commitments, the labelled form above 2^14 cells, l < 64, the host twins.")
    say("staging after the run: %d bytes" % lib.memory_stats()["staging_bytes"])
    lib.srs_release(h)
    lib.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
