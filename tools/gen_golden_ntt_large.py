#!/usr/bin/env python3
"""Fixtures for the three-pass transform sizes no other fixture reaches, 2^25 .. 2^28 (the field's two-adicity), from the REFERENCE
itself (oracle/_ref/libbbref.so, polynomial_arithmetic.cpp's fft family, x86-64 asm path, 8 threads):

  all seven kinds at n = 2^25, 2^26, 2^27, 2^28 on the [0, 2r) input of tools/gen_golden_r4b.py (noncanonical_fast of splitmix64
  NTT_SEED scalars; the constant of the *_with_constant kinds from CONST_SEED): SHA-256 of the output + elements at the seams of
  ntt.hip's three-pass layout (output index k1 + n1 k', n1 = 2^(log2n - 2 (log2n / 3))) and at four seeded random indices.

Inputs are deterministic, so tests/golden/ntt_large.json holds the recipe, digests and sampled elements only, and a second run writes
the same bytes.  Host memory: the input, one working copy and the reference's domain (its root tables): 40 GiB peak at 2^28;
about 10 minutes on 8 threads.
    python tools/gen_golden_ntt_large.py
"""
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.pyoracle import NTT_KINDS, Oracle, Ref, aligned_empty  # noqa: E402
from tests.util import sha_inplace  # noqa: E402
from tools.gen_golden import CONST_SEED, GOLD, NTT_SEED, hx, noncanonical_fast  # noqa: E402

SIZES = (25, 26, 27, 28)
SAMPLE_SEED = 0x5A3D1E5


def sample_indices(log2n):
    """the seams of the three-pass layout (output index k1 + n1 k': k1 < n1 varies fastest) and four seeded random indices"""
    n, n1 = 1 << log2n, 1 << (log2n - 2 * (log2n // 3))
    seams = [0, 1, n1 - 1, n1, n1 + 1, n // 2 - 1, n // 2, n - n1, n - 2, n - 1]
    rng = np.random.Generator(np.random.PCG64(SAMPLE_SEED + log2n))
    rand = [int(v) for v in rng.integers(0, n, size=4)]
    return sorted(set(seams + rand))


def main():
    O, R = Oracle(), Ref(True)
    const = O.random_scalars(CONST_SEED, 1)[0]
    out = {"source": "reference polynomial_arithmetic.cpp fft family via oracle/_ref, 8 threads (tools/gen_golden_ntt_large.py)",
           "input": "noncanonical_fast(random_scalars(ntt_seed, n)): splitmix64 scalars, +r on every third element (index % 3 == 0)",
           "ntt_seed": "0x%x" % NTT_SEED, "constant_seed": "0x%x" % CONST_SEED, "constant": hx(const),
           "sample_seed": "0x%x" % SAMPLE_SEED, "ntt": []}
    t_all = time.time()
    for lg in SIZES:
        n = 1 << lg
        R.set_threads(8)  # also drops the domains of earlier sizes (the reference asserts a power-of-two thread count)
        t0 = time.time()
        co = noncanonical_fast(O.random_scalars(NTT_SEED, n))
        work = aligned_empty((n, 4))
        R.prepare_domain(n)
        print("2^%d input + domain %.1fs" % (lg, time.time() - t0), flush=True)
        idx = sample_indices(lg)
        for kind in NTT_KINDS:
            t0 = time.time()
            np.copyto(work, co)
            R.ntt_inplace(work, kind, const)
            out["ntt"].append({"n": n, "kind": kind, "sha256": sha_inplace(work), "samples": {str(i): hx(work[i]) for i in idx}})
            print("ntt 2^%d %s %.1fs" % (lg, kind, time.time() - t0), flush=True)
        del co, work
    R.set_threads(8)
    with open(os.path.join(GOLD, "ntt_large.json"), "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print("wrote %s: %.1fs, peak RSS %.1f GiB" % (os.path.join(GOLD, "ntt_large.json"), time.time() - t_all,
                                                 resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20))


if __name__ == "__main__":
    main()
