"""What tests/test_plonk_verify_host.py and tests/test_gpu_plonk_verify.py share: the rows of tests/golden/plonk_verify.json (honest and tampered
proofs with the REFERENCE's verdict, tools/gen_plonk_verify_golden.py) as arrays, loaded once, never written to."""
import functools
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFFFFFFFFFF
SEED = np.array([0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x0F1E2D3C4B5A6978, 0x1122334455667788], dtype=np.uint64)
BAD_POINT, ZERO_EVAL = 1, 2


def _words(hexstr):
    return np.array([int(hexstr[16 * i:16 * i + 16], 16) for i in range(len(hexstr) // 16)], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "plonk_verify.json")) as fh:
        g = json.load(fh)
    g2_x = np.array([int(v, 16) for v in g["g2_x"]], dtype=np.uint64)
    circuits = {}
    for key, c in g["circuits"].items():
        vk = np.array([[int(h[16 * (3 - k):16 * (4 - k)], 16) for k in range(4)] for h in c["vk"]], dtype=np.uint64).reshape(-1, 8)
        circuits[key] = dict(n=c["n"], widgets=c["widgets"], vk=vk)
    rows = [dict(circuit=r["circuit"], tamper=r["tamper"], status=r["rule_status"], verdict=r["reference_verdict"], proof=_words(r["proof"]))
            for r in g["rows"]]
    for r in rows:
        r["proof"].setflags(write=False)
    return g2_x, circuits, rows


def row_ids():
    return ["%s-%s" % (r["circuit"], r["tamper"]) for r in fixture()[2]]


def row(circuit, tamper):
    return next(r for r in fixture()[2] if r["circuit"] == circuit and r["tamper"] == tamper)


def fields(rep):
    """a report without its sums and seed"""
    return {k: int(getattr(rep, k)) for k in ("count", "bad_status", "first_bad_status", "pairing_checked", "pairing_ok", "first_bad_proof")}


def whole(rep):
    return dict(fields(rep), seed=[int(v) for v in rep.seed], a=[int(v) for v in rep.a], b=[int(v) for v in rep.b], status=[int(v) for v in rep.status])


def mixed_batch(count, bad):
    """`count` proofs of the 32-gate standard circuit: honest ones, and at the positions of `bad` (position -> tamper name) tampered ones"""
    proofs = np.tile(row("standard/32", "none")["proof"], (count, 1))
    for j, tamper in bad.items():
        proofs[j] = row("standard/32", tamper)["proof"]
    return proofs
