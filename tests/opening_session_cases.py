"""Shared cases of the opening-session tests (tests/test_opening_session_host.py, tests/test_gpu_opening_session.py; test infrastructure, may import
oracle/), over tests/lagrange_open_cases.py: the fold by the oracle's arithmetic (Python integers through PolyOracle.plain / mont), the sets of points a
session is begun with, the sets of multipliers a fold takes, and what a folded opening must give -- the definition of lagrange_open_cases.expected applied
to the folded vector.  The host twins and the GPU entries are judged against the same values."""
import numpy as np

from oracle.pyoracle import FR_MODULUS as R, PolyOracle, aligned_copy, from_int, to_int
from tests.lagrange_open_cases import expected, omega

ERR_STATE = " -4:"


def fold(v, n, batch, stride, gamma):
    """(n, 4): F_i = sum_b gamma_b v_{b,i}, canonical; v (batch * stride, 4), gamma (batch, 4), any representatives"""
    g = PolyOracle.plain(gamma)
    rows = [PolyOracle.plain(v[b * stride:b * stride + n]) for b in range(batch)]
    return aligned_copy(PolyOracle.mont([sum(g[b] * rows[b][i] for b in range(batch)) % R for i in range(n)]))


def folded_expected(oracle, v, n, batch, stride, gamma, z):
    """(F(z) as (4,), the quotient's values as (n, 4)) of the fold"""
    return expected(oracle, fold(v, n, batch, stride, gamma), n, z)


def add(a, b):
    """element-wise sum of two (k, 4) arrays, canonical"""
    return aligned_copy(PolyOracle.mont([x + y for x, y in zip(PolyOracle.plain(a), PolyOracle.plain(b))]))


def on_domain(n, m, lift=False):
    z = PolyOracle.mont([pow(omega(n), m, R)])[0]
    return from_int(to_int(z) + R) if lift and to_int(z) + R < 1 << 256 else z


def point_sets(oracle, n):
    """(name, [(z, m or None), ...]): 1, 2 and 4 points off the domain; every m of {0, 1, 63, 64, n/2, n - 1} below n mixed with points off it, four at
    a time (one of the on-domain points lifted by r); the same point twice, off the domain and on it"""
    off = [(z, None) for z in oracle.random_scalars(0x5E55 + n, 4)]
    out = [("off x%d" % k, off[:k]) for k in (1, 2, 4)]
    ms = sorted({m for m in (0, 1, 63, 64, n // 2, n - 1) if m < n})
    on = [(on_domain(n, m, lift=(j == 1)), m) for j, m in enumerate(ms)]
    for k in range(0, len(on), 2):
        pair = on[k:k + 2]
        out.append(("mixed m=%s" % [m for _, m in pair], [off[0]] + pair + [off[1]][:4 - 1 - len(pair)]))
    out.append(("twice off", [off[2], off[2]]))
    out.append(("twice on", [on[-1], off[3], on[-1]]))
    return out


def gamma_sets(oracle, batch, seed=0x6A3):
    """(name, gamma (batch, 4)): random; all ones; one zero entry; one entry r - 1; a representative gamma + r"""
    rnd = oracle.random_scalars(seed + batch, batch)
    one, last = PolyOracle.mont([1])[0], batch - 1

    def with_entry(k, value):
        g = rnd.copy()
        g[k] = value
        return aligned_copy(g)
    lifted = next((from_int(to_int(g) + R) for g in rnd if to_int(g) + R < 1 << 256), from_int(R))  # (r itself: the representative of zero)
    return [("random", aligned_copy(rnd)), ("ones", aligned_copy(np.tile(one, (batch, 1)))), ("a zero", with_entry(last, from_int(0))),
            ("r - 1", with_entry(0, PolyOracle.mont([R - 1])[0])), ("gamma + r", with_entry(last // 2, lifted))]
