"""What an opening session buys a prover that opens a PLONK-shaped set of polynomials given as values (profiles/opening_session.txt is this tool's
output): one process on one MI355X, both libraries loaded side by side -- the in-tree build (child) and the PARENT commit's build (--parent-lib) -- every
leg warm, the two legs of a cell alternating inside every pair (the order swapped from pair to pair).  Wall milliseconds per CALL SEQUENCE around the C
entries, Python binding included, each leg ended by a device synchronise.  n = 2^16 and 2^20, random values, z random (off the domain), the legacy default
stream, commitments over a bbgpu_srs_lagrange handle of each library's own.
  (1) the PLONK shape: eight polynomials, six opened at z and two at z w, all eight evaluations wanted, one proof point per point.
      parent: two bbgpu_kate_opening_lagrange_device calls (batch 6 and batch 2, f returned) and eight MSMs, one per quotient.
      child:  begin(2 points), two evaluate, two open_folded, a device synchronise (the MSMs run on streams of their own), two MSMs, end.
  (2) the same without the commitments (and without that synchronise).
  (3) one polynomial at one point, evaluation only: child begin + evaluate + end against the parent's bbgpu_fr_evaluate_lagrange_device, and against the
      parent's bbgpu_ntt_device(IFFT) + bbgpu_fr_evaluate_device (in place on a buffer of its own: the copy that keeping the values would cost is not charged).
  (4) no regression: the two existing entries, bbgpu_fr_evaluate_lagrange_device and bbgpu_kate_opening_lagrange_device at batch 1 and 8, parent against child.
  (5) where the child's time of (2) goes: every call of it alone (child only, not paired), and bbgpu_fr_batch_invert_device of 2 n elements for scale --
      begin + end less that inversion is what the session's own allocation costs (hipMalloc, and a hipFree that waits for the device).
No ratio is asserted: the lines say which leg's median is lower and whether the gap exceeds the spread (the slower leg's interquartile range).
Usage: make the parent's library once (barretenberg_amd/csrc: `make variant NAME=parent` in a checkout of the parent, copied to
barretenberg_amd/_variants/libbbgpu_parent.so), then  python tools/opening_session_bench.py [--pairs 21] [--parent-lib PATH] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from barretenberg_amd.plonk import FR_MODULUS, to_montgomery_limbs  # noqa: E402
from tools.lagrange_open_bench import LINES, PARENT_LIB, line, pairs, say, show, timed  # noqa: E402  (the same clock, pairing and report lines)

MONT_INV = pow(1 << 256, -1, FR_MODULUS)
ROOT28 = 0x1860EF942963F9E756452AC01EB203D8A22BF3742445FFD6636E735580D13D9C * MONT_INV % FR_MODULUS  # the 2^28-th root of unity, out of its Montgomery form


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=21)
    ap.add_argument("--parent-lib", default=PARENT_LIB)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opening_session.txt"))
    args = ap.parse_args()
    import torch
    from barretenberg_amd import BbGpu
    if not os.path.exists(args.parent_lib):
        sys.exit("no parent library at %s (see the usage)" % args.parent_lib)
    child = BbGpu(device=0)
    os.environ["BBGPU_LIB"] = args.parent_lib
    parent = BbGpu(device=0)
    del os.environ["BBGPU_LIB"]
    say("# child %s, parent %s; wall ms per leg, ended by a device synchronise: median (min, max, interquartile range) of %d alternating pairs after a warm pair"
        % (child.version(), parent.version(), args.pairs))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x0E55100)
    x = np.array([0x1234567, 0x89ABCDE, 0xF012345, 0x6789AB], dtype=np.uint64)  # any secret: a string nobody uses
    z = np.array([0x0F1E2D3C4B5A6978, 0x1122334455667788, 0x99AABBCCDDEEFF00, 0x0123456789ABCDEF], dtype=np.uint64)
    gamma = np.arange(1, 33, dtype=np.uint64).reshape(8, 4) * np.uint64(0x9E3779B97F4A7C15)  # any multipliers
    for n in (1 << 16, 1 << 20):
        lg = n.bit_length() - 1
        # z w, w the root of the size-n domain: ROOT28^(2^28 / n)
        zw = to_montgomery_limbs([int.from_bytes(z.tobytes(), "little") * MONT_INV % FR_MODULUS * pow(ROOT28, 1 << (28 - lg), FR_MODULUS)])[0]
        zs = np.stack([z, zw])
        h_child, h_parent = child.srs_generate(x, n), parent.srs_generate(x, n)
        hl_child, _, _ = child.srs_lagrange(h_child, n)
        hl_parent, _, _ = parent.srs_lagrange(h_parent, n)
        v = torch.randint(-(1 << 63), (1 << 63) - 1, (8 * n, 4), dtype=torch.int64, device="cuda", generator=gen)
        q, qf = torch.empty_like(v), torch.empty((2 * n, 4), dtype=torch.int64, device="cuda")
        c = v[:n].clone()
        at = [v.data_ptr() + b * n * 32 for b in range(8)]
        qat = [q.data_ptr() + b * n * 32 for b in range(8)]

        def parent_open():
            parent.kate_opening_lagrange_device(at[0], qat[0], n, z, batch=6)
            parent.kate_opening_lagrange_device(at[6], qat[6], n, zw, batch=2)

        def parent_open_commit():
            parent_open()
            for b in range(8):
                parent.msm_device(hl_parent, qat[b], n)

        def child_open(commit=False):
            s = child.lagrange_opening_begin(n, zs)
            child.lagrange_opening_evaluate(s, 0, at[0], n, batch=6)
            child.lagrange_opening_evaluate(s, 1, at[6], n, batch=2)
            child.lagrange_opening_open_folded(s, 0, at[0], n, gamma[:6], qf.data_ptr(), want_f=False)
            child.lagrange_opening_open_folded(s, 1, at[6], n, gamma[6:], qf.data_ptr() + n * 32, want_f=False)
            if commit:
                torch.cuda.synchronize()
                child.msm_device(hl_child, qf.data_ptr(), n)
                child.msm_device(hl_child, qf.data_ptr() + n * 32, n)
            child.lagrange_opening_end(s)

        def child_session_evaluate():
            s = child.lagrange_opening_begin(n, z)
            child.lagrange_opening_evaluate(s, 0, at[0], n)
            child.lagrange_opening_end(s)

        def parent_transform_evaluate():
            parent.ntt_device(c.data_ptr(), n, "ifft")
            parent.evaluate_device(c.data_ptr(), n, z)
        ta, tb = pairs(args.pairs, lambda: child_open(True), parent_open_commit)
        line("(1) PLONK shape + commitments n 2^%d" % lg, "session", ta, "parent", tb)
        ta, tb = pairs(args.pairs, child_open, parent_open)
        line("(2) PLONK shape               n 2^%d" % lg, "session", ta, "parent", tb)
        ta, tb = pairs(args.pairs, child_session_evaluate, lambda: parent.evaluate_lagrange_device(at[0], n, z))
        line("(3) evaluate one polynomial   n 2^%d" % lg, "session", ta, "parent entry", tb)
        ta, tb = pairs(args.pairs, child_session_evaluate, parent_transform_evaluate)
        line("(3) evaluate one polynomial   n 2^%d" % lg, "session", ta, "transform", tb)
        for batch in (1, 8):
            ta, tb = pairs(args.pairs, lambda: child.evaluate_lagrange_device(at[0], n, z, batch=batch), lambda: parent.evaluate_lagrange_device(at[0], n, z, batch=batch))
            line("(4) existing evaluate batch %d n 2^%d" % (batch, lg), "child", ta, "parent", tb)
            ta, tb = pairs(args.pairs, lambda: child.kate_opening_lagrange_device(at[0], qat[0], n, z, batch=batch),
                           lambda: parent.kate_opening_lagrange_device(at[0], qat[0], n, z, batch=batch))
            line("(4) existing open     batch %d n 2^%d" % (batch, lg), "child", ta, "parent", tb)
        s = child.lagrange_opening_begin(n, zs)
        for name, call in (("begin(2 points) + end", lambda: child.lagrange_opening_end(child.lagrange_opening_begin(n, zs))),
                           ("batch inversion of 2 n", lambda: child.lib.bbgpu_fr_batch_invert_device(q.data_ptr(), 2 * n, 0)),
                           ("evaluate batch 6", lambda: child.lagrange_opening_evaluate(s, 0, at[0], n, batch=6)),
                           ("evaluate batch 2", lambda: child.lagrange_opening_evaluate(s, 1, at[6], n, batch=2)),
                           ("open_folded batch 6", lambda: child.lagrange_opening_open_folded(s, 0, at[0], n, gamma[:6], qf.data_ptr(), want_f=False)),
                           ("open_folded batch 2", lambda: child.lagrange_opening_open_folded(s, 1, at[6], n, gamma[6:], qf.data_ptr(), want_f=False))):
            say("(5) alone n 2^%d  %s" % (lg, show("%-24s" % name, [timed(call) for _ in range(args.pairs + 1)][1:])))
        child.lagrange_opening_end(s)
        for lib, handles in ((child, (hl_child, h_child)), (parent, (hl_parent, h_parent))):
            for h in handles:
                lib.srs_release(h)
        del v, q, qf, c
    child.shutdown()
    parent.shutdown()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
