"""Known-answer tests of the DEVICE field and group layer (csrc/fe.hpp with the gfx950 asm products, csrc/g1.hpp) through
bbgpu_selftest_field / bbgpu_selftest_g1: the reference tests' own vectors (tests/golden/reference_kats.json <-
test/test_fq.cpp:51-133, test_fr.cpp:51-88, test_g1.cpp:41-122), outputs of the reference itself (field_ops.json, g1_ops.json)
and the lazy-bound extremes of the 9 x 29-bit representation against exact integer arithmetic.  Bit-exact (integer work)."""
import numpy as np
import pytest

from oracle.pyoracle import FQ, FR, FQ_MODULUS, FR_MODULUS, from_int, to_int
from tests.util import limbs

pytestmark = pytest.mark.gpu

MOD = {"fq": FQ_MODULUS, "fr": FR_MODULUS}
R256 = 1 << 256


@pytest.fixture(scope="module")
def gpu():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.shutdown()


def _ints(arr):
    return [to_int(r) for r in arr]


def _expected(op, a, b, p):
    """value the op names, on Montgomery-2^256 residues: a~ = a R.  Products return (x y) R, i.e. a~ b~ / R."""
    rinv = pow(R256, -1, p)
    mm = lambda x, y: x * y * rinv % p
    return {
        "mul": mm(a, b), "sqr": mm(a, a), "add": (a + b) % p, "sub": (a - b) % p, "neg": (-a) % p,
        "mul_add": (mm(a, b) + mm(a + b, a - b)) % p, "mul_sub": (mm(a, b) - mm(2 * a, b)) % p,
        "lazy_limbs": mm(2 * a, 3 * b), "lazy_weak": mm(4 * a, b - a), "lazy_value": 28 * a % p, "reduce": 28 * a % p,
        "sqr_lazy": mm(2 * a - b, 2 * a - b),
        "mul_addhi": (mm(a, b) - a) % p, "sqr_addhi": (mm(a, a) - b - 2 * a) % p,
    }[op]


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_device_field_ops_vs_reference_outputs(gpu, golden, field):
    """field_ops.json: outputs of the reference's own asm path on the same operands"""
    p = MOD[field]
    cases = [c for c in golden("field_ops.json")["cases"] if c["field"] == field]
    a = np.stack([limbs(c["a"]) for c in cases])
    b = np.stack([limbs(c["b"]) for c in cases])
    for op in ("mul", "sqr", "add", "sub", "neg"):
        got = _ints(gpu.selftest_field(field, op, a, b))
        hits = 0
        for c, g in zip(cases, got):
            if op in c:  # not every case carries every op
                assert g == to_int(limbs(c[op])) % p and g < p, (field, op, c["a"])
                hits += 1
        assert hits >= 4, (field, op)


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_device_field_reference_kats(gpu, golden, field):
    """the hard-coded vectors of test_fq.cpp / test_fr.cpp, including their out-of-range raw operands (any 256-bit value is a
    legal input of the device layer; the device answers with the canonical representative)"""
    p = MOD[field]
    done = 0
    for k in golden("reference_kats.json")[field]:
        if k["op"] not in ("mul", "sqr", "add", "sub"):
            continue
        a = limbs(k["a"]).reshape(1, 4)
        b = limbs(k["b"]).reshape(1, 4) if "b" in k else a
        got = to_int(gpu.selftest_field(field, k["op"], a, b)[0])
        assert got == to_int(limbs(k["expected"])) % p, k["cite"]
        done += 1
    assert done >= 3


@pytest.mark.parametrize("field", ["fq", "fr"])
def test_device_field_lazy_bounds(gpu, oracle, field):
    """every op on random and on extreme operands (0, 1, p - 1, p, 2p - 1, 2^256 - 1, all limbs 2^29 - 1 ...) against exact
    integers: unnormalised limbs at the multiplier's limit (L1 L2 = 6), beyond it (renormalised), values up to 168 p"""
    p = MOD[field]
    rng = np.random.default_rng(20261004)
    special = [0, 1, 2, p - 1, p, p + 1, 2 * p - 1, 2 * p, 5 * p, R256 - 1, R256 - 2, (1 << 255), (1 << 232) - 1,
               sum(((1 << 29) - 1) << (29 * i) for i in range(8)), sum(1 << (29 * i) for i in range(9)) % R256, 0x1FFFFFFF, 1 << 29]
    vals = special + [int.from_bytes(rng.bytes(32), "little") for _ in range(200)]
    pairs = [(x, y) for x in special for y in special[:9]] + list(zip(vals, reversed(vals))) + [(v, v) for v in vals[:40]]
    a = np.stack([from_int(x) for x, _ in pairs])
    b = np.stack([from_int(y) for _, y in pairs])
    for op in ("mul", "sqr", "add", "sub", "neg", "mul_add", "mul_sub", "lazy_limbs", "lazy_weak", "lazy_value", "reduce", "sqr_lazy", "mul_addhi", "sqr_addhi"):
        got = _ints(gpu.selftest_field(field, op, a, b))
        for (x, y), g in zip(pairs, got):
            assert g == _expected(op, x, y, p), (field, op, hex(x), hex(y))
    z = gpu.selftest_field(field, "zero_tests", a, b)
    for (x, y), r in zip(pairs, z):
        assert (int(r[0]) & 1) == int((x - y) % p == 0), (hex(x), hex(y))
        assert (int(r[0]) >> 1 & 1) == int((x - y) * x % p == 0), (hex(x), hex(y))


# ---------------------------------------------------------------------------------------------------------------------
def _norm_xyzz(oracle, r):
    """device result {X, Y, ZZ, ZZZ} -> normalised reference element (12 limbs)"""
    out = np.zeros(12, dtype=np.uint64)
    if not r[8:12].any():
        out[7] = np.uint64(1 << 63)
        return out
    out[0:4] = oracle.mul(FQ, r[0:4], oracle.invert(FQ, r[8:12]))
    out[4:8] = oracle.mul(FQ, r[4:8], oracle.invert(FQ, r[12:16]))
    out[8:12] = oracle.const(FQ, "one")
    # ZZ^3 == ZZZ^2: the pair is a consistent extended-Jacobian denominator
    zz, zzz = r[8:12], r[12:16]
    assert np.array_equal(oracle.mul(FQ, oracle.sqr(FQ, zz), zz), oracle.sqr(FQ, zzz))
    return out


def _norm(oracle, p):
    return oracle.g1_normalize_or_inf(p) if hasattr(oracle, "g1_normalize_or_inf") else oracle.g1_normalize(p)


def _inf():
    p = np.zeros(12, dtype=np.uint64)
    p[7] = np.uint64(1 << 63)
    return p


def test_device_g1_ops_vs_reference_outputs(gpu, oracle, golden):
    """g1_ops.json: mixed_add, add, dbl outputs of the reference's group.hpp on the same operands (compared after normalisation:
    the device uses other coordinates, the affine point is unique)"""
    cases = golden("g1_ops.json")["cases"]
    acc = np.stack([limbs(c["acc"]) for c in cases])
    q = np.stack([limbs(c["scalar_mul_G"]) for c in cases])
    m = np.stack([limbs(c["mixed_add"]) for c in cases])
    a = np.stack([limbs(c["add"]) for c in cases])
    for op, p_in, q_in, key in (("madd", acc, q, "mixed_add"), ("add", m, acc, "add"), ("quad_add", m, acc, "add"), ("dbl", a, a, "dbl")):
        got = gpu.selftest_g1(op, p_in, q_in)
        for c, r in zip(cases, got):
            assert np.array_equal(_norm_xyzz(oracle, r), oracle.g1_normalize(limbs(c[key]))), (op, c["scalar"])
    for c, r in zip(cases, gpu.selftest_g1("dbl", a, a)):
        assert np.array_equal(_norm_xyzz(oracle, r), limbs(c["normalize"]))


def test_device_g1_reference_kats(gpu, oracle, golden):
    """test_g1.cpp:41-122: mixed_add, add and three doublings on the hard-coded points"""
    def mont(d, keys):
        return np.concatenate([oracle.to_mont(FQ, limbs(d[c])) for c in keys])
    done = 0
    for k in golden("reference_kats.json")["g1"]:
        if k["op"] == "mixed_add":
            qa = np.concatenate([mont(k["b"], "xy"), np.zeros(4, dtype=np.uint64)])
            got = gpu.selftest_g1("madd", mont(k["a"], "xyz"), qa)[0]
        elif k["op"] == "add":
            got = gpu.selftest_g1("add", mont(k["a"], "xyz"), mont(k["b"], "xyz"))[0]
        elif k["op"] == "dbl3":
            cur = mont(k["a"], "xyz")
            for _ in range(3):
                cur = _norm_xyzz(oracle, gpu.selftest_g1("dbl", cur, cur)[0])
            assert np.array_equal(cur, oracle.g1_normalize(mont(k["expected"], "xyz"))), k["cite"]
            done += 1
            continue
        else:
            continue
        assert np.array_equal(_norm_xyzz(oracle, got), oracle.g1_normalize(mont(k["expected"], "xyz"))), k["cite"]
        done += 1
    assert done >= 3


def test_device_g1_exceptional_cases(gpu, oracle, golden):
    """test_g1.cpp:124-241 on the device layer: P + P, P + (-P), infinity operands, conditional negation"""
    cases = golden("g1_ops.json")["cases"][:6]
    jac = [limbs(c["dbl"]) for c in cases]                       # non-normalised Jacobian representatives
    aff = [oracle.g1_normalize(j) for j in jac]                  # the same points, z = one
    neg = []
    for a in aff:
        n = a.copy()
        n[4:8] = oracle.neg(FQ, a[4:8])
        neg.append(n)
    P, A, N = np.stack(jac), np.stack(aff), np.stack(neg)
    want_dbl = [oracle.g1_normalize(oracle.g1_dbl(j)) for j in jac]
    # mixed addition: P + P -> doubling branch; P + (-P) -> infinity (both via a negated y and via the negating entry); inf + Q -> Q
    for r, w in zip(gpu.selftest_g1("madd", P, A), want_dbl):
        assert np.array_equal(_norm_xyzz(oracle, r), w)
    for r in gpu.selftest_g1("madd", P, N):
        assert np.array_equal(_norm_xyzz(oracle, r), _inf())
    for r in gpu.selftest_g1("madd_neg", P, A):
        assert np.array_equal(_norm_xyzz(oracle, r), _inf())
    for r, w in zip(gpu.selftest_g1("madd_neg", P, N), want_dbl):  # P - (-P)
        assert np.array_equal(_norm_xyzz(oracle, r), w)
    INF = np.stack([_inf()] * len(jac))
    for r, a in zip(gpu.selftest_g1("madd", INF, A), aff):
        assert np.array_equal(_norm_xyzz(oracle, r), a)
    # mixed addition of two different points, negated: P_i - Q_{i+1}
    Q = np.roll(A, 1, axis=0)
    for r, j, n in zip(gpu.selftest_g1("madd_neg", P, Q), jac, np.roll(N, 1, axis=0)):
        assert np.array_equal(_norm_xyzz(oracle, r), oracle.g1_normalize(oracle.g1_mixed_add(j, n[:8])))
    # full addition: P + P, P + (-P), inf + P, P + inf, inf + inf -- by the one-lane add() and by the four-lane quad addition of the bucket reduction
    for op in ("add", "quad_add"):
        for r, w in zip(gpu.selftest_g1(op, P, A), want_dbl):
            assert np.array_equal(_norm_xyzz(oracle, r), w), op
        for r in gpu.selftest_g1(op, P, N):
            assert np.array_equal(_norm_xyzz(oracle, r), _inf()), op
        for r, a in zip(gpu.selftest_g1(op, INF, P), aff):
            assert np.array_equal(_norm_xyzz(oracle, r), a), op
        for r, a in zip(gpu.selftest_g1(op, P, INF), aff):
            assert np.array_equal(_norm_xyzz(oracle, r), a), op
        for r in gpu.selftest_g1(op, INF, INF):
            assert np.array_equal(_norm_xyzz(oracle, r), _inf()), op
        # two different points, in both orders, mixed with exceptional quads in the same wave
        Qr = np.roll(P, 1, axis=0)
        for r, j, k in zip(gpu.selftest_g1(op, P, Qr), jac, np.roll(np.stack(jac), 1, axis=0)):
            assert np.array_equal(_norm_xyzz(oracle, r), oracle.g1_normalize(oracle.g1_add(j, k))), op
    for r, w in zip(gpu.selftest_g1("add", P, A), want_dbl):
        assert np.array_equal(_norm_xyzz(oracle, r), w)
    for r in gpu.selftest_g1("add", P, N):
        assert np.array_equal(_norm_xyzz(oracle, r), _inf())
    for r, a in zip(gpu.selftest_g1("add", INF, P), aff):
        assert np.array_equal(_norm_xyzz(oracle, r), a)
    for r, a in zip(gpu.selftest_g1("add", P, INF), aff):
        assert np.array_equal(_norm_xyzz(oracle, r), a)
    for r in gpu.selftest_g1("add", INF, INF):
        assert np.array_equal(_norm_xyzz(oracle, r), _inf())
    # doubling: infinity stays infinity; the affine doubling equals the general one
    for r in gpu.selftest_g1("dbl", INF, INF):
        assert np.array_equal(_norm_xyzz(oracle, r), _inf())
    for r, a in zip(gpu.selftest_g1("dbl_affine", A, A), aff):
        assert np.array_equal(_norm_xyzz(oracle, r), oracle.g1_normalize(oracle.g1_dbl(a)))


# ---------------------------------------------------------------------------------------------------------------------
# madd_ip AS COMPILED FOR THE DEVICE: the bucket accumulation's own addition (gfx950 asm products, the limb-0 prefilter in front of the full zero
# test, the two one-sided lane-masked branches, the in-place doubling, infinity as a flag) behind the operand path of msm_accumulate_kernel
# (store_affine_m261 -> load_affine_m261_signed).  The "madd" / "madd_neg" ops above run the plain madd() instead.
def _row(aff, negative=False):
    """operand of the madd_ip ops: affine x, y in limbs 0-7, limb 8 != 0 <=> negative digit"""
    q = np.zeros(12, dtype=np.uint64)
    q[:8] = aff[:8]
    q[8] = 1 if negative else 0
    return q


def _negated(oracle, a):
    n = np.array(a, dtype=np.uint64)
    n[4:8] = oracle.neg(FQ, a[4:8])
    return n


def _norm_flagged(oracle, r):
    assert not (r == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "acc_inf disagrees with is_infinity(acc)"
    return _norm_xyzz(oracle, r)


def _mont_mul(a, b):
    return a * b * pow(R256, -1, FQ_MODULUS) % FQ_MODULUS


def _representative(jac, lam):
    """(X, Y, Z) -> (X lam^2, Y lam^3, Z lam): the same point; all in Montgomery form (raw limbs as ints)"""
    x, y, z = to_int(jac[0:4]), to_int(jac[4:8]), to_int(jac[8:12])
    l2 = _mont_mul(lam, lam)
    return np.concatenate([from_int(_mont_mul(x, l2)), from_int(_mont_mul(y, _mont_mul(l2, lam))), from_int(_mont_mul(z, lam))])


@pytest.fixture(scope="module")
def ip_points(oracle, golden):
    """eight points as non-normalised Jacobian representatives (outputs of the reference's dbl), the same points affine, their negatives, 2 P"""
    cases = golden("g1_ops.json")["cases"][:8]
    jac = [limbs(c["dbl"]) for c in cases]
    aff = [oracle.g1_normalize(j) for j in jac]
    neg = [_negated(oracle, a) for a in aff]
    dbl = [oracle.g1_normalize(oracle.g1_dbl(j)) for j in jac]
    return jac, aff, neg, dbl


def test_device_madd_ip_exceptional_cases(gpu, oracle, ip_points):
    """the operands of test_device_g1_exceptional_cases through the accumulation's madd_ip: generic, P + P, P + (-P) by the sign bit and by a
    negated y, P - (-P), -P - (-P), an infinite accumulator with either sign"""
    jac, aff, neg, dbl = ip_points
    P, INF = np.stack(jac), np.stack([_inf()] * len(jac))
    rows = lambda pts, s: np.stack([_row(a, s) for a in pts])
    norm = lambda out: [_norm_flagged(oracle, r) for r in out]
    other, other_neg = aff[-1:] + aff[:-1], neg[-1:] + neg[:-1]  # P_i meets Q_(i-1)
    for r, j, a in zip(norm(gpu.selftest_g1("madd_ip", P, rows(other, False))), jac, other):
        assert np.array_equal(r, oracle.g1_normalize(oracle.g1_mixed_add(j, a[:8])))
    for r, j, a in zip(norm(gpu.selftest_g1("madd_ip", P, rows(other, True))), jac, other_neg):
        assert np.array_equal(r, oracle.g1_normalize(oracle.g1_mixed_add(j, a[:8])))
    for r, w in zip(norm(gpu.selftest_g1("madd_ip", P, rows(aff, False))), dbl):       # P + P
        assert np.array_equal(r, w)
    for r in norm(gpu.selftest_g1("madd_ip", P, rows(aff, True))):                     # P - P, the sign bit
        assert np.array_equal(r, _inf())
    for r in norm(gpu.selftest_g1("madd_ip", P, rows(neg, False))):                    # P + (-P), y negated beforehand
        assert np.array_equal(r, _inf())
    for r, w in zip(norm(gpu.selftest_g1("madd_ip", P, rows(neg, True))), dbl):        # P - (-P)
        assert np.array_equal(r, w)
    NP = np.stack([np.concatenate([j[0:4], oracle.neg(FQ, j[4:8]), j[8:12]]) for j in jac])  # -P, the same non-normalised representative
    for r in norm(gpu.selftest_g1("madd_ip", NP, rows(neg, True))):                    # -P - (-P)
        assert np.array_equal(r, _inf())
    for r, w in zip(norm(gpu.selftest_g1("madd_ip", NP, rows(neg, False))), dbl):      # -P + (-P) = -(2 P)
        assert np.array_equal(r, _negated(oracle, w))
    for r, a in zip(norm(gpu.selftest_g1("madd_ip", INF, rows(aff, False))), aff):     # inf + Q: the loop's start branch
        assert np.array_equal(r, a)
    for r, n in zip(norm(gpu.selftest_g1("madd_ip", INF, rows(aff, True))), neg):      # inf - Q
        assert np.array_equal(r, n)


def test_device_madd_ip_every_representative(gpu, oracle, ip_points):
    """P + P and P - P on 256 representatives (X l^2, Y l^3, Z l) of each of eight accumulators: P = x2 ZZ1 - X1 is a different multiple of p for
    every l, so its lazily reduced square PP lands on whichever of 0, p, 2p that l gives -- the values the limb-0 prefilter has to let through"""
    jac, aff, neg, dbl = ip_points
    rng = np.random.default_rng(20261017)
    reps, idx = [], []
    for i, j in enumerate(jac):
        for _ in range(256):
            reps.append(_representative(j, int.from_bytes(rng.bytes(32), "little") % (FQ_MODULUS - 1) + 1))
            idx.append(i)
    reps = np.stack(reps)
    for operands, sign, doubles in ((aff, False, True), (aff, True, False), (neg, False, False), (neg, True, True)):
        q = np.stack([_row(operands[i], sign) for i in idx])
        out = gpu.selftest_g1("madd_ip", reps, q)
        for k, (i, r) in enumerate(zip(idx, out)):
            assert np.array_equal(_norm_flagged(oracle, r), dbl[i] if doubles else _inf()), (i, k % 256, sign, doubles)


def test_device_madd_ip_exceptional_lanes_inside_a_wave(gpu, oracle, ip_points):
    """one 64-lane wave in which a few lanes double, cancel or start while the others add two different points -- the two one-sided branches of
    madd_ip and the start branch under partial lane masks -- with the exceptional lanes at the wave's edges, its middle and next to each other"""
    jac, aff, neg, dbl = ip_points
    m = len(jac)
    for places in ((0,), (63,), (0, 63), (31, 32), (1, 2, 3, 17, 40, 62), tuple(range(0, 64, 2)), tuple(range(64))):
        p_in, q_in, want = [], [], []
        for lane in range(64):
            i = lane % m
            if lane in places:
                kind = places.index(lane) % 4
                if kind == 0:    # P + P
                    p_in.append(jac[i]); q_in.append(_row(aff[i], False)); want.append(dbl[i])
                elif kind == 1:  # P - P
                    p_in.append(jac[i]); q_in.append(_row(aff[i], True)); want.append(_inf())
                elif kind == 2:  # inf - Q
                    p_in.append(_inf()); q_in.append(_row(aff[i], True)); want.append(neg[i])
                else:            # P - (-P)
                    p_in.append(jac[i]); q_in.append(_row(neg[i], True)); want.append(dbl[i])
            else:
                k, s = (i + 1 + lane // m) % m, lane % 3 == 0
                if k == i:
                    k = (i + 1) % m
                p_in.append(jac[i]); q_in.append(_row(aff[k], s))
                want.append(oracle.g1_normalize(oracle.g1_mixed_add(jac[i], (neg[k] if s else aff[k])[:8])))
        out = gpu.selftest_g1("madd_ip", np.stack(p_in), np.stack(q_in))
        for lane, (r, w) in enumerate(zip(out, want)):
            assert np.array_equal(_norm_flagged(oracle, r), w), (places, lane)


def test_device_madd_ip_chains(gpu, oracle, golden):
    """chains of 256 signed operands from {G, 2G, 4G, Q} folded as a chunk of the accumulation folds them, the accumulator carried in place from trip
    to trip.  Three chains: a scripted prefix -- G + G (a doubling), + 2G (a doubling of the doubled sum), - 4G (a cancellation), a restart, another
    cancellation and restart -- followed by a seeded +-G walk whose sums k G keep returning to 0 and +-1 and which is steered home so that the LAST
    step cancels; its mirror image; and a walk over all eight operands.  ONE launch, six lanes per j = 0 .. 255: lanes 6j + c fold the first j + 1
    operands of chain c (all 256 prefixes of every chain), lanes 6j + 3 + c a window of chain c that starts somewhere else and wraps.  Neighbouring
    lanes therefore hold different sums and meet different operands at the same trip: the test first checks, from the scalars alone, that in the
    first wave there are trips at which lanes start, add, double AND cancel side by side.  Every lane against k G from its scalar sum (Q = q G
    with the fixture's q)"""
    from tests.colliding import MONT, R, closed_form_point
    G = oracle.g1_one_affine()
    c = golden("g1_ops.json")["cases"][3]
    q_scalar, Q = to_int(limbs(c["scalar"])), limbs(c["scalar_mul_G"])[:8]
    g2 = oracle.g1_normalize(oracle.g1_dbl(np.concatenate([G, oracle.const(FQ, "one")])))
    g4 = oracle.g1_normalize(oracle.g1_dbl(g2))
    ops = {1: (G, MONT), 2: (g2[:8], 2 * MONT % R), 4: (g4[:8], 4 * MONT % R), "Q": (Q, q_scalar)}  # affine point, raw scalar
    m = 256
    rng = np.random.default_rng(4)
    prefix = [(1, 1), (1, 1), (2, 1), (4, -1), ("Q", 1), ("Q", -1), (4, -1), (4, -1), (4, 1), (4, 1)]  # sums G 2G 4G 0 Q 0 -4G -8G -4G 0
    walk, k = list(prefix), 0
    while len(walk) < m:
        left = m - len(walk)
        s = (-1 if k > 0 else 1) if abs(k) >= left else (1 if rng.integers(0, 2) else -1)  # |k| steps left: straight home
        walk.append((1, s))
        k += s
    assert k == 0 and len(walk) == m
    mixed = list(prefix) + [((1, 2, 4, "Q")[rng.integers(0, 4)], 1 if rng.integers(0, 2) else -1) for _ in range(m - len(prefix))]
    chains = [walk, [(o, -s) for o, s in walk], mixed]
    flat = [e for ch in chains for e in ch]                      # chain c = rows [c m, (c + 1) m)
    value = [s * ops[o][1] % R for o, s in flat]                 # the scalar of every signed operand
    n = 6 * m
    lanes = []                                                   # (start, count, ring begin, ring end)
    for j in range(m):
        lanes += [(cc * m, j + 1, cc * m, (cc + 1) * m) for cc in range(3)]
        lanes += [(cc * m + (37 * j + 11 + 5 * cc) % m, 1 + (101 * j + 7 + 3 * cc) % m, cc * m, (cc + 1) * m) for cc in range(3)]

    def sequence(lane):
        start, count, lo, hi = lane
        return [lo + (start - lo + t) % (hi - lo) for t in range(count)]

    # what the lanes of the first wave do at each trip, from the scalars alone (k G = k' G <=> k = k' mod r)
    richest = 0
    seqs = [sequence(l) for l in lanes[:64]]
    sums = [0] * 64
    fresh = [True] * 64
    for t in range(m):
        kinds = set()
        for l, sq in enumerate(seqs):
            if t >= len(sq):
                continue
            v = value[sq[t]]
            kind = "start" if fresh[l] or sums[l] == 0 else "double" if sums[l] == v else "cancel" if (sums[l] + v) % R == 0 else "add"
            kinds.add(kind)
            sums[l] = (sums[l] + v) % R
            fresh[l] = False
        richest = max(richest, len(kinds))
    assert richest == 4, richest

    p = np.zeros((n, 12), dtype=np.uint64)
    p[:, :4] = np.array(lanes, dtype=np.uint64)
    q = np.zeros((n, 12), dtype=np.uint64)
    q[:3 * m] = np.stack([_row(ops[o][0], s < 0) for o, s in flat])
    out = gpu.selftest_g1("madd_ip_chain", p, q)
    points, zeros = {}, 0
    for i, (lane, r) in enumerate(zip(lanes, out)):
        total = sum(value[x] for x in sequence(lane)) % R
        if total not in points:
            points[total] = closed_form_point(oracle, total)
        zeros += total == 0
        assert np.array_equal(_norm_flagged(oracle, r), points[total]), (i, lane)
    assert zeros >= 16, zeros  # lanes that END on a cancellation
    for cc in (0, 1):          # the walk and its mirror end at infinity: their last step cancels
        assert sum(value[cc * m:(cc + 1) * m]) % R == 0
    # a lane description out of range is answered with all-ones, not with a read outside the operands
    bad = p.copy()
    bad[0, :4] = (0, 1, 0, n + 1)
    bad[1, :4] = (5, 1, 6, 9)
    bad[2, :4] = (0, 4097, 0, m)
    out = gpu.selftest_g1("madd_ip_chain", bad, q)
    assert all((out[i] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() for i in range(3)) and not (out[3] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
