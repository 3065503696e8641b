"""Shared cases of the tests of evaluation and opening in evaluation form (tests/test_lagrange_open_host.py, tests/test_gpu_lagrange_open.py; test
infrastructure, may import oracle/): the values, the points z and what the entries must give.  Every expected value goes through the coefficient form:
f(z) = PolyOracle.evaluate(ifft v, z) and the quotient is fft(PolyOracle.kate_opening(ifft v, z)) -- the definition the issue gives, with the oracle's
transforms -- except at z = 0, where the reference's recurrence divides by -z: there the quotient is the coefficients shifted down by one, in Python
integers.  The host twins and the GPU entries are judged against the same values."""
import numpy as np

from oracle.pyoracle import FR_MODULUS as R, PolyOracle, aligned_copy, from_int, to_int

ERR_SIZE, ERR_ARG = " -2:", " -3:"
PAD = 0x5A5A5A5A5A5A5A5A  # what the elements between the polynomials hold


def omega(n):
    return PolyOracle.root(n.bit_length() - 1)


def values(oracle, seed, n, batch=1, stride=None):
    """(batch * stride, 4): random values, elements 1 and n - 1 of every polynomial lifted by r (representatives at or above r that still fit 256 bits);
    the elements between the polynomials hold PAD"""
    stride = n if stride is None else stride
    out = np.full((batch * stride, 4), PAD, dtype=np.uint64)
    rnd = oracle.random_scalars(seed, batch * n).reshape(batch, n, 4)
    for b in range(batch):
        out[b * stride:b * stride + n] = rnd[b]
        for i in {1, n - 1}:
            v = to_int(out[b * stride + i])
            if v + R < 1 << 256:
                out[b * stride + i] = from_int(v + R)
    return aligned_copy(out)


def canonical(v):
    return aligned_copy(PolyOracle.mont(PolyOracle.plain(v)))


def z_cases(oracle, n, extra_m=()):
    """(name, z as (4,) uint64, m or None): random, 0, r (the representative of zero), 1, -1, w^(n-1), w^m + r for an m in the middle, w^(n/2 + 1) (n > 2),
    and w^m for every m of extra_m"""
    w = omega(n)

    def on(m, lift=False):
        z = PolyOracle.mont([pow(w, m, R)])[0]
        return from_int(to_int(z) + R) if lift else z
    mid = n // 2 + 1 if n > 2 else 1
    lifted = next(m for m in (n // 3 + 1, 1, 0) if m < n and to_int(on(m)) + R < 1 << 256)
    out = [("random", oracle.random_scalars(0x2E3 + n, 1)[0], None), ("zero", from_int(0), None), ("r", from_int(R), None), ("one", on(0), 0),
           ("minus one", on(n // 2), n // 2), ("w^(n-1)", on(n - 1), n - 1), ("w^%d + r" % lifted, on(lifted, True), lifted), ("w^%d" % mid, on(mid), mid)]
    out += [("w^%d" % m, on(m), m) for m in extra_m if m < n]
    return out


def expected(oracle, v, n, z):
    """(f(z) as (4,), quotient values as (n, 4)) of ONE polynomial given by n values (any representatives)"""
    c = oracle.ntt(canonical(v), "ifft")
    fz = PolyOracle.evaluate(c, z)
    if to_int(z) % R == 0:
        q = np.concatenate([c[1:], np.zeros((1, 4), dtype=np.uint64)])
    else:
        q, fz2 = PolyOracle.kate_opening(c, z)
        assert np.array_equal(fz, fz2)
    return fz, oracle.ntt(aligned_copy(q), "fft")


def expected_batch(oracle, v, n, batch, stride, z):
    """(f (batch, 4), quotient in the layout of v with the elements between the polynomials as they were)"""
    f = np.zeros((batch, 4), dtype=np.uint64)
    q = v.copy()
    for b in range(batch):
        f[b], q[b * stride:b * stride + n] = expected(oracle, v[b * stride:b * stride + n], n, z)
    return f, q
