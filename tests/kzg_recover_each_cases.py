"""Shared cases of the tests of bbgpu_kzg_recover_cells_each (tests/test_kzg_recover_each_host.py, tests/test_gpu_kzg_recover_each.py; test infrastructure,
may import oracle/): the call arguments of polynomials that each hold their OWN cells, from the seeded polynomials, the shuffled cell lists and the
plain-integer interpolation of tests/kzg_recover_cells_cases.py."""
import numpy as np

from tests.kzg_recover_cells_cases import R, interpolate, listed_values, memory, polynomial, present_cells

NONE = 0xFFFFFFFFFFFFFFFF  # first_bad of a polynomial that has none


def spread(m, mu, seed=3):
    """mu of the m cells, seeded, ascending"""
    return sorted(int(k) for k in np.random.default_rng([0x3B4E, m, mu, seed]).permutation(m)[:mu])


def each_case(n, l, d, missing_by_poly):
    """polynomial b of degree d - 1 misses missing_by_poly[b] -> (cells, integer value lists, polynomials): cells[b] shuffled with a seed of its own"""
    polys = [polynomial(n, d, b) for b in range(len(missing_by_poly))]
    cells = [present_cells(n, l, missing, seed=2 + b) for b, missing in enumerate(missing_by_poly)]
    ints = [listed_values(v, n, l, c) for (_, v), c in zip(polys, cells)]
    return cells, ints, polys


def each_values(ints, l):
    """the wrapper's `values`: one (count_b, l, 4) array per polynomial"""
    return [memory(v).reshape(-1, l, 4) for v in ints]


def expected_each(coeffs_by_poly, d, cells, l, m):
    """(report, first_bad) the definition gives for the recovered coefficient lists"""
    first = []
    for c, k in zip(coeffs_by_poly, cells):
        bad = [i for i in range(d, len(k) * l) if c[i] % R]
        first.append(bad[0] if bad else NONE)
    rep = dict(consistent=1, first_bad_poly=0, first_bad_coeff=0, max_missing=max(m - len(k) for k in cells))
    for b, f in enumerate(first):
        if f != NONE:
            rep.update(consistent=0, first_bad_poly=b, first_bad_coeff=f)
            break
    return rep, np.array(first, dtype=np.uint64)


__all__ = ["NONE", "R", "each_case", "each_values", "expected_each", "interpolate", "memory", "spread"]
