"""What bbgpu_srs_check costs on one MI355X, against what the library could already do (profiles/srs_check.txt is this tool's output):
per size, wall milliseconds (median / min of `--reps` calls after two warm ones) of
  check          bbgpu_srs_check, honest table, fixed seed, no LOCATE
  locate         the same table with one row negated, BBGPU_SRS_CHECK_LOCATE (the rounds of the bisection included)
  two_msm        two bbgpu_msm_g1_device_async calls in flight over n - 1 resident scalars at offsets 0 and 1 of the same handle, both waited for
  pairing_check  bbgpu_host_pairing_check of two pairs alone (host, no GPU)
and the check's excess over the two MSMs.  Usage: python tools/srs_check_bench.py [--sizes 65536,1048576] [--reps 9]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    import torch
    from barretenberg_amd import BbGpu
    G = BbGpu(device=0)
    rng = np.random.default_rng(7)
    x = np.array([rng.integers(0, 1 << 63, dtype=np.uint64) for _ in range(3)] + [np.uint64(rng.integers(0, 1 << 59))], dtype=np.uint64)
    seed = np.arange(1, 5, dtype=np.uint64)
    fd, tiny_path = tempfile.mkstemp(suffix=".dat")
    os.close(fd)
    _, tiny = G.srs_generate(x, 2, want_host_table=True)
    G.write_transcript(tiny_path, tiny, 2, x)
    g2_x = G.transcript_read_g2(tiny_path)
    os.unlink(tiny_path)
    print("# %s; wall ms, median / min of %d" % (G.version(), args.reps))
    for n in [int(s) for s in args.sizes.split(",")]:
        h, table = G.srs_generate(x, n, want_host_table=True)
        honest = G.srs_check(h, n, g2_x, seed)
        assert honest.ok, honest.as_dict()
        check = timed(lambda: G.srs_check(h, n, g2_x, seed), args.reps)
        d = torch.from_numpy(rng.integers(0, 1 << 61, size=(n - 1, 4), dtype=np.uint64).view(np.int64)).cuda()
        torch.cuda.synchronize()

        def two():
            ta = G.msm_device_async(h, d.data_ptr(), n - 1, offset=0)
            tb = G.msm_device_async(h, d.data_ptr(), n - 1, offset=1)
            G.msm_wait(ta)
            G.msm_wait(tb)
        two_msm = timed(two, args.reps)
        ps = np.stack([np.array(list(honest.a), dtype=np.uint64), np.array(list(honest.b), dtype=np.uint64)])
        qs = np.stack([g2_x, g2_x])
        pairing = timed(lambda: G.host_pairing_check(ps, qs), args.reps)
        k = n // 3
        p = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
        edited = table.copy()  # a table of its own: the address-keyed cache would serve the generated table's resident copy for its host copy
        y = sum(int(v) << (64 * i) for i, v in enumerate(edited[2 * k, 4:8]))
        edited[2 * k, 4:8] = [((p - y) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
        hb = G.srs_register(edited)
        bad = G.srs_check(hb, n, g2_x, seed, locate=True)
        assert not bad.ok and bad.first_bad_power == k - 1, bad.as_dict()
        locate = timed(lambda: G.srs_check(hb, n, g2_x, seed, locate=True), max(3, args.reps // 3))
        print("n %8d  check %8.3f / %8.3f  two_msm %8.3f / %8.3f  excess %+8.3f  pairing_check %7.3f / %7.3f  locate %9.3f / %9.3f" %
              (n, check[0], check[1], two_msm[0], two_msm[1], check[0] - two_msm[0], pairing[0], pairing[1], locate[0], locate[1]))
        G.srs_release(hb)
        G.srs_release(h)
    G.shutdown()


if __name__ == "__main__":
    main()
