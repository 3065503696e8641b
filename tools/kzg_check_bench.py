"""What bbgpu_kzg_check_open_all and bbgpu_kzg_check_openings cost (profiles/kzg_check.txt is this tool's output, below the kernels' resource lines): one
process on one MI355X, every leg warm.  Wall milliseconds per CALL around the C entries, Python binding included; every call ends synchronised (it
returns the verdict).  Claims: one polynomial of n = 256, 4096, 2^16 and 2^20 random coefficients over a generated string, committed to
(bbgpu_msm_g1_device), evaluated (bbgpu_ntt_device) and opened at every domain point (bbgpu_kzg_open_all_device) by the device; fixed seed, no LOCATE;
every report is checked to say ok.
  open-all    bbgpu_kzg_check_open_all(batch 1, n): one shared commitment, z made on the device: 96 bytes per claim cross the link
  per-claim   bbgpu_kzg_check_openings(which = NULL) over the same claims, the commitment repeated and z = omega^i explicit: 192 bytes per claim
  stages      bbgpu_kzg_check_last_timing: uploads + k_kzg_claims + the findings' read-back | k_kzg_fold | the two MSMs | the host tail (two
              normalisations and the pairing check); medians over the same calls
  before      the only check the library had: bbgpu_host_kzg_check_openings in chunks of 64 claims, timed on a SAMPLE of chunks of the same claims in
              the same process and SCALED to count / 64 chunks (an extrapolation; the chunks are independent calls)
Usage: python tools/kzg_check_bench.py [--reps 9] [--chunks 8] [--sizes 256,4096,65536,1048576]"""
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


def show(ts):
    q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
    return "%9.3f (min %9.3f max %9.3f iqr %7.3f)" % (statistics.median(ts), min(ts), max(ts), q[2] - q[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--sizes", default="256,4096,65536,1048576")
    args = ap.parse_args()
    import pathlib
    import tempfile

    import torch
    from barretenberg_amd import BbGpu
    from oracle.pyoracle import Oracle, PolyOracle, aligned_copy, build
    from tests.kzg_check_cases import g2_of, secret_x
    build()
    oracle, lib = Oracle(), BbGpu(device=0)
    sizes = [int(s) for s in args.sizes.split(",")]
    x = secret_x(oracle)
    g2_x = g2_of(lib, oracle, pathlib.Path(tempfile.mkdtemp()), x, "x.dat")
    h = lib.srs_generate(x, max(sizes))
    print("# %s; wall ms per CALL: median (min, max, interquartile range) of %d calls after a warm one; the host path: %d chunks of 64 claims, scaled"
          % (lib.version(), args.reps, args.chunks))
    for n in sizes:
        c = aligned_copy(oracle.random_scalars(0xBE7C + n, n))
        d_c = torch.from_numpy(c.view(np.int64)).cuda()
        setup = lib.kzg_open_all_setup(h, n)
        proofs = lib.kzg_open_all_device(setup, d_c.data_ptr(), n)[0]
        lib.kzg_open_all_release(setup)
        d_y = d_c.clone()
        torch.cuda.synchronize()
        commitment = lib.msm_device(h, d_c.data_ptr(), n)[:8].reshape(1, 8).copy()
        lib.ntt_device(d_y.data_ptr(), n, "fft")
        torch.cuda.synchronize()
        values = d_y.cpu().numpy().view(np.uint64).reshape(n, 4).copy()
        X = np.zeros((n, 4), dtype=np.uint64)  # the polynomial X: its values over the domain are omega^i
        X[1] = PolyOracle.mont([1])[0]
        d_z = torch.from_numpy(aligned_copy(X).view(np.int64)).cuda()
        lib.ntt_device(d_z.data_ptr(), n, "fft")
        torch.cuda.synchronize()
        z = d_z.cpu().numpy().view(np.uint64).reshape(n, 4).copy()
        expanded = np.ascontiguousarray(np.tile(commitment, (n, 1)))
        del d_c, d_y, d_z

        def leg(call):
            total, stages = [], {k: [] for k in STAGES}
            for k in range(args.reps + 1):
                t0 = time.perf_counter()
                rep = call()
                t1 = time.perf_counter()
                assert rep["ok"] == 1, rep
                if k:
                    total.append((t1 - t0) * 1e3)
                    ms = lib.kzg_check_last_timing()
                    for s in STAGES:
                        stages[s].append(ms[s])
            return total, {s: statistics.median(v) for s, v in stages.items()}

        for name, call in (("open-all ", lambda: lib.kzg_check_open_all(commitment, values, proofs, n, g2_x, seed=SEED)),
                           ("per-claim", lambda: lib.kzg_check_openings(expanded, z, values, proofs, g2_x, seed=SEED))):
            total, st = leg(call)
            print("claims %8d  %s  %s   upload + k_kzg_claims %8.3f  fold %6.3f  msms %8.3f  host tail %6.3f" %
                  (n, name, show(total), st["claims_ms"], st["fold_ms"], st["msm_ms"], st["host_tail_ms"]), flush=True)
        chunks = max(1, min(args.chunks, n // 64))
        per = []
        for k in range(chunks + 1):
            lo = (k * 2731 * 64) % max(n - 63, 1)
            sl = slice(lo, lo + min(64, n))
            t0 = time.perf_counter()
            ok = lib.host_kzg_check_openings(expanded[sl], z[sl], values[sl], proofs[sl], g2_x, seed=SEED)
            t1 = time.perf_counter()
            assert ok
            if k:
                per.append((t1 - t0) * 1e3)
        calls = (n + 63) // 64
        print("claims %8d  before     %9.3f = %d calls of bbgpu_host_kzg_check_openings x %s per call of 64, %d timed" %
              (n, calls * statistics.median(per), calls, show(per), len(per)), flush=True)
    print("staging after the run: %d bytes" % lib.memory_stats()["staging_bytes"])
    lib.srs_release(h)
    lib.shutdown()


if __name__ == "__main__":
    main()
