"""The plain statements of the prover's round kernels (tests/plonk_round_cases.py) pinned WITHOUT the code under test: on a random circuit that
satisfies its gates and copy constraints the quotient numerator they describe vanishes at every constrained row, and stops doing so at the row where one
of q_c, q_bo, a sigma entry or q_o_next is broken.  That fixes the signs, the alpha factors, k1 / k2 and the i + 4 wraps of the statements before
tests/test_gpu_plonk_rounds.py lets them judge a kernel.  No GPU: integer arithmetic only.

The statements are evaluated with the coset shift set to 1, so index 4j of a 4n vector and 2j of a 2n vector are row j itself (x = w_n^j); the other
indices hold random values that no checked index reads."""
import random

import numpy as np
import pytest

from oracle.pyoracle import FR, PolyOracle
from tests import plonk_round_cases as cases
from tests.plonk_round_cases import K1, K2, R

N = 16
WIRE_K = (1, K1, K2)
# copy cycles over (row, wire), wire 0 / 1 / 2 = l / r / o, spanning all three wires; the last row takes part in none (rows 0 .. n-2 are constrained)
CYCLES = [[(0, 0), (3, 1), (7, 2)], [(1, 0), (2, 0), (5, 2), (9, 1)], [(4, 1), (6, 2)], [(8, 0), (10, 2), (11, 1), (12, 0)], [(13, 0), (14, 2)]]
BOOL_POSITIONS = {(13, 0): 1, (14, 2): 1, (14, 0): 0, (13, 1): 1, (1, 2): 0, (11, 2): 1}  # wires that hold 0 or 1: the bool selectors are live there
SEQ_ROWS = (2, 5, 9)


def test_generators_match_the_oracle(oracle):
    """k1 = g = 5, k2 = 7 (fr.hpp:65-79), against the oracle's constants -- not against the product's GEN5 / GEN7"""
    assert PolyOracle.plain(oracle.const(FR, "generator"))[0] == cases.K1 == cases.COSET_G == 5
    assert PolyOracle.plain(oracle.const(FR, "alt_generator"))[0] == cases.K2 == 7


class Circuit:
    """a random satisfying circuit of N rows in plain values, and the vectors the statements read"""

    def __init__(self, seed=0x5EED):
        rnd = random.Random(seed)
        f = lambda: rnd.randrange(R)
        n, w = N, PolyOracle.root(cases.log2(N))
        self.w = [[f() for _ in range(n)] for _ in range(3)]  # [wire][row]
        for (j, t), bit in BOOL_POSITIONS.items():
            self.w[t][j] = bit
        for cyc in CYCLES:
            for j, t in cyc[1:]:
                self.w[t][j] = self.w[cyc[0][1]][cyc[0][0]]
        # sigma: the identity, then every cycle rotated by one position; as field elements k_wire * w^row (permutation.hpp:15-87)
        nxt = {(j, t): (j, t) for j in range(n) for t in range(3)}
        for cyc in CYCLES:
            for a, b in zip(cyc, cyc[1:] + cyc[:1]):
                nxt[a] = b
        self.sigma = [[WIRE_K[nxt[(j, t)][1]] * pow(w, nxt[(j, t)][0], R) % R for j in range(n)] for t in range(3)]
        self.qm, self.ql, self.qr, self.qo = ([f() for _ in range(n)] for _ in range(4))
        self.qon = [f() if j in SEQ_ROWS else 0 for j in range(n)]
        self.qb = [[f() if (j, t) in BOOL_POSITIONS else 0 for j in range(n)] for t in range(3)]
        wl, wr, wo = self.w
        # the extended gate: q_m w_l w_r + q_l w_l + q_r w_r + q_o w_o + q_c + q_o_next w_o[next row] = 0, solved for q_c: live and full-width
        self.qc = [-(self.qm[j] * wl[j] * wr[j] + self.ql[j] * wl[j] + self.qr[j] * wr[j] + self.qo[j] * wo[j] + self.qon[j] * wo[(j + 1) % n]) % R
                   for j in range(n)]
        self.beta, self.gamma, self.alpha, self.abase, self.cl, self.cr, self.co = (f() for _ in range(7))
        # Z: z_terms and the exclusive prefix products of num / den (prover.cpp:194-202)
        num, den = cases.z_terms(wl, wr, wo, *self.sigma, self.beta, self.gamma, n)
        ratio = [a * pow(b, -1, R) % R for a, b in zip(num, den)]
        self.z = PolyOracle.plain(PolyOracle.product_scan(PolyOracle.mont(ratio)))
        self.rnd = rnd

    def spread(self, rows, k):
        """a vector of k * N entries with row j at index k j and random values between"""
        out = [self.rnd.randrange(R) for _ in range(k * N)]
        out[::k] = rows
        return out

    def numerator(self, sigma=None, qc=None, qbo=None, qon=None):
        """the quotient numerator at the rows: QUOT_LARGE at 4j plus QUOT_MID, QUOT_SEQ and QUOT_BOOL accumulated at 2j"""
        n, (wl, wr, wo) = N, self.w
        sigma = sigma or self.sigma
        wl4, wr4, wo4 = (self.spread(v, 4) for v in self.w)
        s4 = [self.spread([(wires[j] + self.beta * sg[j] + self.gamma) % R for j in range(n)], 4) for wires, sg in zip(self.w, sigma)]  # prover.cpp:253-269
        zf = self.spread([self.alpha * v % R for v in self.z], 4)
        large = cases.quot_large(wl4, wr4, wo4, *s4, zf, self.beta, self.gamma, 4 * n, shift=1)
        l1 = self.spread([1] + [0] * (n - 1), 2)  # L_1 at the rows
        sel = [self.spread(v, 2) for v in (self.qm, self.ql, self.qr, self.qo, qc or self.qc)]
        mid = cases.quot_mid(zf, wl4, wr4, wo4, l1, *sel, self.alpha, self.abase, 2 * n)
        # sequential_widget.cpp:49: the sequential term carries the arithmetic widget's own alpha power
        mid = cases.quot_seq(mid, wo4, self.spread(qon or self.qon, 2), self.abase, 2 * n)
        qb = [self.spread(v, 2) for v in (self.qb[0], self.qb[1], qbo or self.qb[2])]
        mid = cases.quot_bool(mid, wl4, wr4, wo4, *qb, self.cl, self.cr, self.co, 2 * n)
        return [(large[4 * j] + mid[2 * j]) % R for j in range(n)]


@pytest.fixture(scope="module")
def circuit():
    return Circuit()


def test_circuit_is_what_the_issue_asks_for(circuit):
    c = circuit
    assert all(v >> 200 for v in c.qc[:N - 1]) and all(v >> 200 for v in c.qm + c.ql + c.qr + c.qo), "q_c and the selectors are full-width"
    assert sum(1 for v in c.qb[2] if v) >= 2 and sum(1 for v in c.qon if v) == len(SEQ_ROWS)
    assert c.z[0] == 1 and len(set(c.z)) > N // 2, "a grand product that moves"
    assert c.z[N - 1] * 1 % R == 1, "the copy cycles close inside rows 0 .. n-2"
    assert {t for cyc in CYCLES for _, t in cyc} == {0, 1, 2}


def test_numerator_vanishes_on_a_satisfying_circuit(circuit):
    assert circuit.numerator()[:N - 1] == [0] * (N - 1)


def _only_row(values, row):
    return values[row] != 0 and all(v == 0 for j, v in enumerate(values[:N - 1]) if j != row)


def test_broken_q_c_shows_at_its_row(circuit):
    qc = list(circuit.qc)
    qc[3] = (qc[3] + 1) % R
    assert _only_row(circuit.numerator(qc=qc), 3)


def test_broken_q_bo_shows_at_its_row(circuit):
    qbo = list(circuit.qb[2])
    assert qbo[0] == 0 and circuit.w[2][0] not in (0, 1)
    qbo[0] = 1  # the output wire of row 0 is no boolean
    assert _only_row(circuit.numerator(qbo=qbo), 0)


def test_broken_sigma_shows_at_its_row(circuit):
    sigma = [list(s) for s in circuit.sigma]
    sigma[0][8] = K2 * pow(PolyOracle.root(cases.log2(N)), 4, R) % R  # (8, l) now points at (4, o), which holds another value
    assert sigma[0][8] != circuit.sigma[0][8]
    assert _only_row(circuit.numerator(sigma=sigma), 8)


def test_broken_q_o_next_shows_at_its_row(circuit):
    qon = list(circuit.qon)
    qon[5] = (qon[5] + 1) % R
    assert circuit.w[2][6] != 0
    assert _only_row(circuit.numerator(qon=qon), 5)


def test_mimc_statement_vanishes_on_a_mimc_chain():
    """mimc_widget.cpp: T = w_o + w_l + coefficient, w_r = T^3, next w_o = w_r^2 T; the selector full-width, off at the last row (its next row wraps)"""
    n, rnd = 8, random.Random(0x313C)
    f = lambda: rnd.randrange(R)
    key, coef = f(), [f() for _ in range(n)]
    wl, wr, wo = [key] * n, [0] * n, [f()] + [0] * (n - 1)
    for j in range(n):
        t = (wo[j] + wl[j] + coef[j]) % R
        wr[j] = t * t * t % R
        if j + 1 < n:
            wo[j + 1] = wr[j] * wr[j] * t % R
    qsel = [f() for _ in range(n - 1)] + [0]
    spread = lambda rows: [v for r in rows for v in (r, f(), f(), f())]
    abase, astep = f(), f()

    def at_rows(coef_rows):
        out = cases.quot_mimc([0] * (4 * n), spread(wl), spread(wr), spread(wo), spread(qsel), spread(coef_rows), abase, astep, 4 * n)
        return out[::4]
    assert at_rows(coef) == [0] * n
    broken = list(coef)
    broken[2] = (broken[2] + 1) % R
    got = at_rows(broken)
    assert got[2] != 0 and all(v == 0 for j, v in enumerate(got) if j != 2)


@pytest.mark.parametrize("n_src,n_target", [(8, 16), (8, 32), (4, 16), (256, 1024)])
def test_divide_vanishing_by_index_is_the_oracle_walk(oracle, n_src, n_target):
    c = oracle.random_scalars(0xD171DE + n_target, n_target)
    want = PolyOracle.divide_by_pseudo_vanishing(c, n_src, n_target)
    assert np.array_equal(PolyOracle.mont(cases.divide_vanishing(PolyOracle.plain(c), n_src, n_target)), want)
    some = [0, 1, n_target - 1, n_target // 2]
    assert np.array_equal(PolyOracle.mont(cases.divide_vanishing(cases.Rows(c), n_src, n_target, some)), want[some])


def test_scan_statements_agree_with_the_oracle(oracle):
    v, z = oracle.random_scalars(0x5CA9, 37), oracle.random_scalars(0x5CAA, 1)
    pv, pz = PolyOracle.plain(v), PolyOracle.plain(z)[0]
    incl, excl = cases.horner_suffix(pv, pz, True), cases.horner_suffix(pv, pz, False)
    assert np.array_equal(PolyOracle.mont([incl[0]])[0], PolyOracle.evaluate(v, z)) and cases.evaluate(pv, pz) == incl[0]
    assert excl[-1] == 0 and all((excl[i] * pz + pv[i]) % R == incl[i] for i in range(37)) and excl[:-1] == incl[1:]
    # the opening quotient of polynomial_arithmetic.cpp:562-591 is the exclusive scan
    assert np.array_equal(PolyOracle.kate_opening(v, z)[0][:-1], PolyOracle.mont(excl)[:-1])
    assert np.array_equal(PolyOracle.mont([cases.product_of(pv)])[0], PolyOracle.product_scan(v, inclusive=True)[-1])


def test_inputs_cover_the_admitted_range(oracle):
    """what the GPU tests feed: every lane of every vector holds the six raw extremes, every second vector only the largest representatives"""
    vs = cases.input_vectors(oracle, 7, 3, 2, [9, 18, 9])
    assert [v.shape for v in vs] == [(18, 4), (36, 4), (18, 4)]
    ints = [[int.from_bytes(row.tobytes(), "little") for row in v] for v in vs]
    for k, v in enumerate(ints):
        per = len(v) // 2
        for l in range(2):
            assert {0, R - 1, R, 2 * R, 5 * R, (1 << 256) - 1} <= set(v[l * per:(l + 1) * per]), (k, l)
    assert sum(1 for x in ints[1] if x + R >= 1 << 256) >= len(ints[1]) - 12 and sum(1 for x in ints[0] if x < R) > 9
    plain, mont = cases.challenges(oracle, 7, 3, 2)
    assert plain[2] == [0, R - 1] and plain[1] == [R - 1, 0] and PolyOracle.plain(mont) == [v for row in plain for v in row]
    assert all(int.from_bytes(row.tobytes(), "little") < R for row in mont)


def test_entry_refuses_before_it_touches_a_device():
    """bbgpu_selftest_plonk_round checks its arguments on the host: the same refusals as tests/test_gpu_plonk_rounds.py, on a machine without a GPU"""
    from barretenberg_amd import BbGpu
    from barretenberg_amd.bbgpu import BbGpuError
    g = BbGpu(init=False)
    z = np.zeros((1 << 10, 4), dtype=np.uint64)
    for kernel, lanes, length, nin, consts, params in cases.REFUSED:
        with pytest.raises(BbGpuError, match="error -3"):
            g.selftest_plonk_round(kernel, lanes, length, [z] * nin, consts=consts, params=params)
