"""Shared cases of the tests of the batched check of KZG openings (tests/test_kzg_check_host.py, tests/test_gpu_kzg_check.py; test infrastructure, may
import oracle/).  Claims come from a known secret: the string is honest_table(secret_x), commitments are bbgpu_host_msm_g1 of the coefficients, the proofs
at the domain points are bbgpu_host_kzg_open_all's (held to the quotient definition by tests/test_kzg_open_all_host.py), the proofs off the domain are the
commitment of bbgpu_host_kate_opening's quotient, the values are the host transform's.  Nothing here calls the entries under test."""
import numpy as np

from oracle.pyoracle import FQ, FR, FR_MODULUS as R, aligned_copy, from_int, to_int
from tests.kzg_open_all_cases import INF, domain
from tests.srs_check_cases import SEED, g2_of  # noqa: F401  (re-exported)
from tests.srs_update_cases import honest_table, secret_x

ERR_SIZE, ERR_ARG = " -2:", " -3:"
NONE = 0xFFFFFFFFFFFFFFFF
SCALARS = ("count", "bad_points", "first_bad", "first_bad_is_proof", "g2_ok", "ok", "rounds", "first_failing")


def honest(count, **kw):
    """the scalar fields of the report of `count` true claims"""
    return dict(dict(count=count, bad_points=0, first_bad=NONE, first_bad_is_proof=0, g2_ok=1, ok=1, rounds=1, first_failing=-1), **kw)


def scalars(report):
    return {k: report[k] for k in SCALARS}


def make_world(lib, oracle, tmp_path, n, batch):
    """`batch` polynomials of n coefficients over the string of secret_x, opened at every point of the size-n domain: table (2n, 8), g2_x, coeffs
    (batch, n, 4), commitments (batch, 8), values (batch, n, 4), proofs (batch, n, 8), z (n, 4).  Polynomial 1 (if there is one) is constant: its
    proofs are all at infinity.  Made once per module, never written to."""
    x = secret_x(oracle)
    table = honest_table(oracle, x, n)
    coeffs = aligned_copy(oracle.random_scalars(0xC1A1 + 131 * n + batch, batch * n)).reshape(batch, n, 4)
    if batch > 1:
        coeffs[1, 1:] = 0
    coeffs = aligned_copy(coeffs)
    commitments = np.stack([lib.host_msm(aligned_copy(coeffs[b]), table, n)[:8] for b in range(batch)])
    if n == 1:  # constants: the value is the coefficient, the quotient is zero
        proofs, values = np.tile(INF, (batch, 1, 1)), coeffs.copy()
    else:
        proofs = lib.host_kzg_open_all(table, n, aligned_copy(coeffs.reshape(-1, 4)), batch=batch)
        values = np.stack([lib.host_ntt(aligned_copy(coeffs[b]), "fft") for b in range(batch)])
    if batch > 1:
        assert np.array_equal(proofs[1], np.tile(INF, (n, 1)))
    return dict(n=n, batch=batch, table=table, g2_x=g2_of(lib, oracle, tmp_path, x, "x.dat"), coeffs=coeffs, commitments=commitments, values=values,
                proofs=proofs, z=domain(oracle, n))


def off_domain_claim(lib, oracle, W, b, seed):
    """(z, y, pi) of polynomial b at a random point: the quotient's commitment over the same rows"""
    z = oracle.random_scalars(0x0FFD + seed, 1)[0]
    q, y = lib.host_kate_opening(aligned_copy(W["coeffs"][b]), z)
    return z, y, lib.host_msm(aligned_copy(q), W["table"], W["n"])[:8]


def claims_of(W, count, start=0):
    """`count` true claims in the shared layout drawn from the world's batch x n, in an order that mixes the polynomials: (which, z, y, proofs)"""
    n, batch = W["n"], W["batch"]
    assert count <= n * batch
    t = np.arange(start, start + count)
    b, i = t % batch, (t * 7 + t // batch) % n
    return b.astype(np.uint32), aligned_copy(W["z"][i]), aligned_copy(W["values"][b, i]), aligned_copy(W["proofs"][b, i])


def expanded(W, which):
    """the per-claim layout's commitments of a shared call"""
    return aligned_copy(W["commitments"][which])


def plus_one(oracle, v):
    return oracle.add(FR, v, oracle.const(FR, "one"))


def above_r(v):
    """the same residue as the representative in [r, 2r)"""
    out = from_int(to_int(v) + R)
    assert R <= to_int(out) < 2 * R
    return out


def off_curve(oracle, p):
    """a finite point with one added to y"""
    q = np.array(p, dtype=np.uint64).copy()
    q[4:] = oracle.add(FQ, q[4:], oracle.const(FQ, "one"))
    return q


def negated(oracle, p):
    """-P: on the curve, another point"""
    q = np.array(p, dtype=np.uint64).copy()
    q[4:] = oracle.neg(FQ, q[4:])
    return q
