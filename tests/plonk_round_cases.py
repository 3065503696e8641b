"""Plain statements of the prover's round kernels (csrc/poly.hip) over Python integers modulo r, written from the formulas of the reference's
prover.cpp:135-222, 224-300, 302-403, 461-463, 520-528, arithmetic_widget.cpp:66-104, bool_widget.cpp:62-100, sequential_widget.cpp:47-62 and
mimc_widget.cpp:58-90 -- no Montgomery form, no 2^5 repair factor, no table of powers -- plus the inputs the GPU tests feed the kernels
(tests/test_gpu_plonk_rounds.py).  tests/test_plonk_round_refs_host.py pins these statements on a satisfying circuit, without the code under test.

Vectors are anything indexable that yields plain residues (a list, or a Rows over an array too long to convert in full); every function takes the
indices to evaluate (default: all) and returns a list of plain values in that order."""
import numpy as np

from oracle.pyoracle import FR_MODULUS, PolyOracle
from tests.util import extreme_positions, lift_extremes, lift_max

R = FR_MODULUS
# fr.hpp:65-79: the coset generator g (also k1 of the permutation argument) and k2; tests/test_plonk_round_refs_host.py checks them against oracle.const
K1, K2, COSET_G = 5, 7, 5


def log2(n):
    assert n > 0 and n & (n - 1) == 0, n
    return n.bit_length() - 1


class Rows:
    """plain residues of single rows of an (n, 4) Montgomery array, converted when asked for (the 2^21-element cases read a few thousand rows)"""

    def __init__(self, a):
        self.a, self.seen = a, {}

    def __getitem__(self, i):
        if i not in self.seen:
            self.seen[i] = PolyOracle.plain(self.a[i])[0]
        return self.seen[i]


def _idx(idx, n):
    return range(n) if idx is None else idx


# ---- the grand product ------------------------------------------------------------------------------------------------------------------------------
def z_terms(w_l, w_r, w_o, s1, s2, s3, beta, gamma, n, idx=None):
    """prover.cpp:148-187, x = w_n^i -> (num, den)"""
    w, num, den = PolyOracle.root(log2(n)), [], []
    for i in _idx(idx, n):
        x = pow(w, i, R)
        num.append((w_l[i] + beta * x + gamma) * (w_r[i] + beta * K1 * x + gamma) * (w_o[i] + beta * K2 * x + gamma) % R)
        den.append((w_l[i] + beta * s1[i] + gamma) * (w_r[i] + beta * s2[i] + gamma) * (w_o[i] + beta * s3[i] + gamma) % R)
    return num, den


# ---- the quotient ---------------------------------------------------------------------------------------------------------------------------------
def quot_large(wl, wr, wo, s1, s2, s3, zf, beta, gamma, n4, idx=None, shift=COSET_G):
    """prover.cpp:294-299, 310-341 on the 4n coset, x = g w_4n^i; index i + 4 is the next gate's row (:286-289 wraps it)"""
    w, out = PolyOracle.root(log2(n4)), []
    for i in _idx(idx, n4):
        x = shift * pow(w, i, R) % R
        ident = (wl[i] + beta * x + gamma) * (wr[i] + beta * K1 * x + gamma) * (wo[i] + beta * K2 * x + gamma) % R * zf[i]
        out.append((ident - s1[i] * s2[i] * s3[i] % R * zf[(i + 4) % n4]) % R)
    return out


def quot_mid(zf, wl, wr, wo, l1, qm, ql, qr, qo, qc, alpha, abase, n2, idx=None):
    """prover.cpp:360-402 and arithmetic_widget.cpp:86-101 on the 2n coset; zf and the wires are 4n vectors, read at 2i"""
    out = []
    for i in _idx(idx, n2):
        a, b, c = wl[2 * i], wr[2 * i], wo[2 * i]
        gate = qm[i] * a * b + ql[i] * a + qr[i] * b + qo[i] * c + qc[i]
        out.append(((zf[(2 * i + 4) % (2 * n2)] - alpha) * alpha * l1[(i + 4) % n2] + (zf[2 * i] - alpha) * alpha * alpha * l1[i] + abase * gate) % R)
    return out


def quot_seq(q, wo, qon, c, n2, idx=None):
    """sequential_widget.cpp:47-62: q[i] += c q_o_next[i] w_o[2i + 4]"""
    return [(q[i] + c * qon[i] * wo[(2 * i + 4) % (2 * n2)]) % R for i in _idx(idx, n2)]


def quot_bool(q, wl, wr, wo, qbl, qbr, qbo, cl, cr, co, n2, idx=None):
    """bool_widget.cpp:62-100: q[i] += sum over the three wires of c_w q_bw[i] (w^2 - w), wires at 2i"""
    out = []
    for i in _idx(idx, n2):
        a, b, c = wl[2 * i], wr[2 * i], wo[2 * i]
        out.append((q[i] + cl * qbl[i] * (a * a - a) + cr * qbr[i] * (b * b - b) + co * qbo[i] * (c * c - c)) % R)
    return out


def quot_mimc(q, wl, wr, wo, qsel, qcoef, abase, astep, n4, idx=None):
    """mimc_widget.cpp:58-90 on the 4n coset, T = w_o + w_l + q_coef"""
    out = []
    for i in _idx(idx, n4):
        t = (wo[i] + wl[i] + qcoef[i]) % R
        out.append((q[i] + abase * qsel[i] * ((t * t * t - wr[i]) + astep * (wr[i] * wr[i] * t - wo[(i + 4) % n4]))) % R)
    return out


def divide_vanishing(c, n_src, n_target, idx=None):
    """polynomial_arithmetic.cpp:478-560 by its formula, index by index: c[i] (x - w_n^-1) / (x^n - 1), x = g w_N^i.  PolyOracle.divide_by_pseudo_vanishing
    is the same walked in sequence; the host test holds the two against each other"""
    w, last, out = PolyOracle.root(log2(n_target)), pow(PolyOracle.root(log2(n_src)), -1, R), []
    for i in _idx(idx, n_target):
        x = COSET_G * pow(w, i, R) % R
        out.append(c[i] * (x - last) % R * pow(pow(x, n_src, R) - 1, -1, R) % R)
    return out


# ---- the small pointwise kernels ------------------------------------------------------------------------------------------------------------------
def lincomb(ps, cs, addend=None):
    """prover.cpp:520-528, arithmetic_widget.cpp:106-126: sum_j c_j p_j[i] (+ addend[i])"""
    return [(sum(c * p[i] for c, p in zip(cs, ps)) + (addend[i] if addend is not None else 0)) % R for i in range(len(ps[0]))]


def mul2c(a, b, c):
    return [x * y * c % R for x, y in zip(a, b)]


def sigma_prepare(sigma, w, gamma, n_dst):
    """prover.cpp:253-269: sigma(X) + w(X) + gamma in coefficient form (gamma joins the constant term), zeros up to n_dst"""
    out = [(s + v) % R for s, v in zip(sigma, w)]
    out[0] = (out[0] + gamma) % R
    return out + [0] * (n_dst - len(out))


def copy_pad_scaled(src, c, n_dst):
    return [c * v % R for v in src] + [0] * (n_dst - len(src))


def add_vectors(a, b):
    return [(x + y) % R for x, y in zip(a, b)]


def horner_suffix(v, z, inclusive):
    """out_i = sum_{j >= i} v_j z^(j - i) (inclusive) or sum_{j > i} v_j z^(j - i - 1): polynomial_arithmetic.cpp:562-591 as a scan"""
    out, acc = [0] * len(v), 0
    for i in range(len(v) - 1, -1, -1):
        if inclusive:
            acc = (acc * z + v[i]) % R
            out[i] = acc
        else:
            out[i] = acc
            acc = (acc * z + v[i]) % R
    return out


def product_of(v):
    acc = 1
    for x in v:
        acc = acc * x % R
    return acc


def evaluate(v, z):
    acc = 0
    for x in reversed(v):
        acc = (acc * z + x) % R
    return acc


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def raw_rows(values):
    """(k, 4) uint64 of raw 256-bit integers (no Montgomery conversion, no reduction)"""
    return np.array([[(v >> (64 * l)) & 0xFFFFFFFFFFFFFFFF for l in range(4)] for v in values], dtype=np.uint64)


def input_vectors(oracle, seed, count, lanes, per_lane):
    """`count` lane-major vectors of lanes * per_lane[k] elements (per_lane: one length, or one per vector): oracle.random_scalars; every second vector
    lifted to the largest representatives below 2^256; the six raw extremes of the input range written into every lane of every vector, each vector
    starting at another of them so that no index holds zero in all vectors at once"""
    per_lane = [per_lane] * count if isinstance(per_lane, int) else list(per_lane)
    extremes, out = raw_rows(lift_extremes(R)), []
    for k in range(count):
        n = per_lane[k]
        v = np.array(oracle.random_scalars(seed + 0x9E37 * k, lanes * n)).reshape(lanes, n, 4)
        if k % 2 == 1:
            lift_max(v.reshape(-1, 4), R)
        for l in range(lanes):
            for e, pos in enumerate(extreme_positions(n, len(extremes))):
                v[l, pos] = extremes[(e + k + l) % len(extremes)]
        out.append(v.reshape(-1, 4))
    return out


def challenges(oracle, seed, lanes, k):
    """(plain values [lane][j], the (lanes * k, 4) canonical Montgomery array): random, and from two lanes on the last lane alternates 0 and r - 1,
    from three on the one before it r - 1 and 0"""
    plain = [list(row) for row in np.array(PolyOracle.plain(oracle.random_scalars(seed ^ 0xC4A11E46E5, lanes * k)), dtype=object).reshape(lanes, k)]
    if lanes >= 2:
        plain[lanes - 1] = [0 if j % 2 == 0 else R - 1 for j in range(k)]
    if lanes >= 3:
        plain[lanes - 2] = [R - 1 if j % 2 == 0 else 0 for j in range(k)]
    return plain, PolyOracle.mont([v for row in plain for v in row])


# ---- what bbgpu_selftest_plonk_round refuses (BBGPU_ERR_ARG, on the host): (kernel, lanes, len, input vectors, constants, params) ------------------------
def _c(k):
    return np.zeros((k, 4), dtype=np.uint64)


REFUSED = [
    ("mul2c", 0, 8, 2, None, ()), ("mul2c", 17, 8, 2, _c(17), ()), ("mul2c", -1, 8, 2, None, ()),           # lanes outside 1 .. 16
    ("mul2c", 1, 0, 2, _c(1), ()),                                                                           # no elements
    ("no_such_kernel", 1, 8, 2, _c(1), ()),
    ("z_terms", 1, 12, 6, _c(2), ()), ("quot_large", 1, 12, 7, _c(2), ()), ("quot_mid", 1, 12, 10, _c(2), ()),  # a length that is no power of two where the
    ("quot_seq", 1, 12, 3, _c(1), ()), ("quot_bool", 1, 12, 7, _c(3), ()), ("quot_mimc", 1, 12, 6, _c(2), ()),  # kernel masks indices or takes a root of unity
    ("divide_vanishing", 1, 12, 1, None, (1, 12)),
    ("quot_large", 1, 2, 7, _c(2), ()), ("quot_mid", 1, 1, 10, _c(2), ()),                                   # shorter than the 4n / 2n domain of one gate
    ("divide_vanishing", 1, 16, 1, None, (3, 16)), ("divide_vanishing", 1, 2, 1, None, (2, 2)),              # N / n above 4, n below 1
    ("divide_vanishing", 2, 16, 1, None, (1, 8)), ("add_inplace", 2, 16, 2, None, (8, 16)),                  # a stride shorter than the vector: lanes overlap
    ("add_inplace", 2, 16, 2, None, (16, 8)),
    ("sigma_prepare", 1, 16, 2, _c(1), (8,)), ("copy_pad", 1, 16, 1, None, (8, 0)),                          # a destination shorter than the source
    ("copy_pad", 1, 16, 1, None, (32, 1)), ("copy_pad", 1, 16, 1, _c(1), (32, 0)),                           # scaled without a constant, plain with one
    ("copy_pad", 16, 16, 1, None, ((1 << 18) + 1, 0)),                                                       # lanes x elements above 2^22
    ("lincomb", 1, 16, 13, _c(13), (13, 0)), ("lincomb", 1, 16, 0, None, (0, 0)),                            # count outside 1 .. 12
    ("lincomb", 1, 16, 2, _c(3), (3, 0)), ("lincomb", 1, 16, 3, _c(3), (3, 1)), ("lincomb", 1, 16, 3, _c(3), (3,)),  # vectors / parameters missing
    ("scan", 1, 16, 1, None, (0, 3)), ("scan", 1, 16, 1, None, (2, 4)), ("scan", 1, 16, 1, None, (0, 16 + 4)),  # neither output; unknown mode, flag
    ("scan", 1, 16, 1, None, (1, 4)), ("scan", 1, 16, 1, _c(1), (0, 4)),                                     # Horner without z, products with one
    ("evaluate", 2, 16, 1, _c(2), (2, 0, 2)), ("evaluate", 2, 16, 1, _c(2), (2, 0)),                         # a zidx outside nz, a job without one
    ("evaluate", 1, 16, 1, None, (0, 0)), ("evaluate", 1, 16, 1, _c(17), (17, 0)),
    ("mul2c", 1, 8, 2, raw_rows([R]), ()), ("mul2c", 1, 8, 2, raw_rows([(1 << 256) - 1]), ()),              # a challenge is a reduced value
    ("mul2c", 1, 8, 2, _c(2), ()), ("mul2c", 1, 8, 2, None, ()), ("mul2c", 1, 8, 3, _c(1), ()), ("mul2c", 1, 8, 1, _c(1), ()),
    ("mul2c", 1, 8, 2, _c(1), (1,)),                                                                         # a parameter the kernel does not take
]
