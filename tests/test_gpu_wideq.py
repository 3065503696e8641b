"""The wide quotient digits of the field multiplier (csrc/fe.hpp: digits 0..7 of the Montgomery reduction are full 32-bit products, the top digit keeps
its mask) as compiled for the device (-m gpu).

  * every wide form (mul, sqr, a b + c d, the two in-place forms, the two addhi forms) through the raw-limb ops of bbgpu_selftest_field: the device
    result against the SAME code compiled for the host (tests/cpp/fe_wideq_twin.cpp), limb for limb -- operands at the corners of what a form accepts (limbs at the class maximum,
    0, p - 1, every multiple k p up to the value bound, addends with unnormalised limbs) and 4,096 seeded pairs per form; the host result is checked
    against Python's integers on the way (tests/cpp/test_fe_wideq.cpp does that exhaustively, with the column bound);
  * chains of 256 operands carried in place through the four in-place shapes, device against host;
  * madd_ip on accumulators given as random representatives, P + P, P - P and an infinite accumulator at chosen lanes of a wave whose other lanes add
    ordinary points.  The wide form leaves every value bound where it was (the quotient stays below 2^261 (1 + 2^-26)), so PP still lands on 0, p or
    2 p: the representatives make it land on each;
  * one MSM of 2^10 points with window tables and one without, against the host bucket code;
  * transforms at 2^4 (unfused kernel), 2^10 and 2^11 (the two tile instances), all kinds, on [0, 2r) and max-lift inputs, against the oracle.
The kernels take the wide digits in Fq only (fe.hpp Digits / F::WIDE_DIGITS); the Fr forms are generated and are tested here as forms."""
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FQ, FQ_MODULUS, FR_MODULUS, NTT_KINDS, aligned_copy, from_int, to_int
from tests.test_gpu_ntt_sizes import canonical_residues, check_equal, input_classes
from tests.util import CONST_SEED, NTT_SEED, SCALAR_SEED, SRS_SEED, limbs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NL, M29, U, MAXV = 9, (1 << 29) - 1, (1 << 29) + 8, 168
MOD = {"fq": FQ_MODULUS, "fr": FR_MODULUS}
FORMS = ("wide_mul", "wide_sqr", "wide_mul2", "wide_mul_ip", "wide_mul2_ip", "wide_mul_addhi_ip", "wide_sqr_addhi")
TWO = ("wide_mul2", "wide_mul2_ip")
ADDHI = ("wide_mul_addhi_ip", "wide_sqr_addhi")
SQR = ("wide_sqr", "wide_sqr_addhi")


@pytest.fixture(scope="module")
def gpu():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    g.set_host_thresholds(0, 0)  # every size on the device kernels
    yield g
    g.shutdown()


@pytest.fixture(scope="module")
def host_twin(tmp_path_factory):
    """tests/cpp/fe_wideq_twin.cpp: the function the device self-test runs per lane, compiled for the host -> callable (field, op, ac, bd) -> (cases, 9)"""
    from barretenberg_amd import BbGpu
    d = tmp_path_factory.mktemp("wideq_twin")
    exe = str(d / "fe_wideq_twin")
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "fe_wideq_twin.cpp"), "-o", exe], check=True)

    def run(field, op, ac, bd):
        m = ac.shape[0]
        rows = np.zeros((2, m, 24), dtype=np.uint32)
        rows[0, :, :18] = ac
        rows[1, :, :18] = bd
        rows.tofile(str(d / "in.bin"))
        subprocess.run([exe, field, str(BbGpu.SELFTEST_FIELD_OPS[op]), str(d / "in.bin"), str(d / "out.bin")], check=True)
        return np.fromfile(str(d / "out.bin"), dtype=np.uint32).reshape(m, 24)[:, :9].copy()
    return run


# ---- operands of the madd_ip op (the layout tests/test_gpu_selftest.py documents) ----
R256 = 1 << 256


def inf_point():
    p = np.zeros(12, dtype=np.uint64)
    p[7] = np.uint64(1 << 63)
    return p


def row(aff, negative=False):
    """affine x, y in limbs 0-7, limb 8 != 0 <=> negative digit"""
    q = np.zeros(12, dtype=np.uint64)
    q[:8] = aff[:8]
    q[8] = 1 if negative else 0
    return q


def negated(oracle, a):
    n = np.array(a, dtype=np.uint64)
    n[4:8] = oracle.neg(FQ, a[4:8])
    return n


def norm_xyzz(oracle, r):
    """device result {X, Y, ZZ, ZZZ} -> normalised reference element (12 limbs); ZZ = 0: infinity.  All-ones: the flag disagreed with the accumulator"""
    assert not (r == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "acc_inf disagrees with is_infinity(acc)"
    if not r[8:12].any():
        return inf_point()
    out = np.zeros(12, dtype=np.uint64)
    out[0:4] = oracle.mul(FQ, r[0:4], oracle.invert(FQ, r[8:12]))
    out[4:8] = oracle.mul(FQ, r[4:8], oracle.invert(FQ, r[12:16]))
    out[8:12] = oracle.const(FQ, "one")
    return out


def representative(jac, lam):
    """(X, Y, Z) -> (X lam^2, Y lam^3, Z lam): the same point; all in Montgomery form"""
    mont = lambda a, b: a * b * pow(R256, -1, FQ_MODULUS) % FQ_MODULUS
    x, y, z = to_int(jac[0:4]), to_int(jac[4:8]), to_int(jac[8:12])
    l2 = mont(lam, lam)
    return np.concatenate([from_int(mont(x, l2)), from_int(mont(y, mont(l2, lam))), from_int(mont(z, lam))])


@pytest.fixture(scope="module")
def ip_points(oracle, golden):
    """eight points as non-normalised Jacobian representatives (outputs of the reference's dbl), the same points affine, their negatives, 2 P"""
    cases = golden("g1_ops.json")["cases"][:8]
    jac = [limbs(c["dbl"]) for c in cases]
    aff = [oracle.g1_normalize(j) for j in jac]
    neg = [negated(oracle, a) for a in aff]
    dbl = [oracle.g1_normalize(oracle.g1_dbl(j)) for j in jac]
    return jac, aff, neg, dbl


def exact(v):
    return [(v >> (29 * i)) & M29 if i < NL - 1 else v >> (29 * i) for i in range(NL)]


def lift(d, L):
    """the same value with limbs pushed into class L: (L - 1) 2^29 moved down from limb i + 1 wherever it can lend it"""
    d, k = list(d), L - 1
    for i in range(NL - 1):
        if d[i + 1] >= k and d[i] + (k << 29) < L * U:
            d[i + 1] -= k
            d[i] += k << 29
    return d


def value(d):
    return sum(int(x) << (29 * i) for i, x in enumerate(d))


def corner_operands(p, L):
    """(limbs, V) with V the smallest bound value < V p, or V = 0 for the all-limbs-at-maximum operand (no field value: columns only)"""
    vals = [0, p - 1] + [k * p for k in range(1, MAXV)] + [k * p - 1 for k in (1, 2, 3, 12, 13, 22, MAXV)]
    out = [(lift(exact(v), L), v // p + 1) for v in vals]
    out.append(([L * U - 1] * NL, 0))
    return out


def addends(p):
    return [(exact(0), 1), (exact(13 * p), 14), (lift(exact(13 * p), 3), 14), (lift(exact(28 * p - 1), 5), 28), (lift(exact(28 * p - 1), 7), 28),
            ([0xFFFFFFFF] * NL, 0)]


def mul_v(v1, v2):
    return v1 * v2 // 169 + 2


def build_cases(field, form, rng):
    """rows (a, b, c, d_or_e) of limb lists, and per row the declared value bound of the result (0: not a field value, compared with the host only)"""
    p = MOD[field]
    ops = {L: corner_operands(p, L) for L in (1, 2, 3, 4)}
    adds = addends(p)
    zero = ([0] * NL, 1)
    cases = []

    def put(a, b, c=zero, d=zero, e=None):
        valued = all(x[1] for x in (a, b, c, d)) and (e is None or e[1])
        v = 0
        if valued:
            v = (a[1] * b[1] + c[1] * d[1]) // 169 + 2 if form in TWO else mul_v(a[1], b[1])
            v += e[1] if e is not None else 0
            if v > MAXV:
                return  # the typed layer refuses the pair
        cases.append((a[0], b[0], c[0], (e if e is not None else d)[0], v))

    if form in SQR:
        for L in (1, 2):
            for i, a in enumerate(ops[L]):
                for e in (adds if form in ADDHI else [None]):
                    put(a, a, e=e)
    elif form in TWO:
        for q in ((1, 1, 1, 1), (1, 2, 1, 2), (2, 1, 1, 2), (1, 3, 1, 1), (1, 1, 3, 1)):
            a, b, c, d = (ops[L] for L in q)
            n = len(a)
            for i in range(n):
                for j in range(3):
                    put(a[i], b[(i * 7 + j * 31) % n], c[(i * 3 + j * 17 + 1) % n], d[(i * 5 + j * 11 + 2) % n])
            put(a[-1], b[-1], c[-1], d[-1])
    else:
        for la, lb in ((1, 1), (1, 2), (1, 3), (2, 2), (1, 4), (4, 1)):
            a, b = ops[la], ops[lb]
            n = len(a)
            for i in range(n):
                for j in (i, 0, 1, 2, n - 9, n - 8, n - 1, (i * 7 + 3) % n):
                    put(a[i], b[j], e=adds[(i + j) % len(adds)] if form in ADDHI else None)
    # 4,096 seeded pairs: values below 2^256 (what unpack() delivers: V = 6), limbs lifted into a random admissible class
    classes = ((1, 1, 1, 1), (1, 2, 1, 2), (1, 3, 1, 1), (2, 1, 2, 1)) if form in TWO else ((1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (1, 4), (4, 1))
    if form in SQR:
        classes = ((1, 1), (2, 2))
    for k in range(4096):
        cl = classes[k % len(classes)]
        vs = [int.from_bytes(rng.bytes(32), "little") for _ in range(4)]
        o = [(lift(exact(v), cl[i % len(cl)]), v // p + 1) for i, v in enumerate(vs)]
        if form in SQR:
            put(o[0], o[0], e=(lift(exact(vs[3]), 1 + k % 7), vs[3] // p + 1) if form in ADDHI else None)
        elif form in TWO:
            put(o[0], o[1], o[2], o[3])
        else:
            put(o[0], o[1], e=(lift(exact(vs[3]), 1 + k % 7), vs[3] // p + 1) if form in ADDHI else None)
    return cases


@pytest.mark.parametrize("field", ("fq", "fr"))
def test_wide_forms_device_equals_host_limb_for_limb(gpu, host_twin, field):
    p = MOD[field]
    rng = np.random.default_rng(20261019)
    for form in FORMS:
        cases = build_cases(field, form, rng)
        assert len(cases) >= 4096 + 300, (form, len(cases))
        ac = np.array([c[0] + c[2] for c in cases], dtype=np.uint32)
        bd = np.array([c[1] + c[3] for c in cases], dtype=np.uint32)
        host = host_twin(field, form, ac, bd)
        dev = gpu.selftest_field_raw(field, form, ac, bd)
        bad = np.nonzero((host != dev).any(axis=1))[0]
        assert bad.size == 0, (field, form, int(bad[0]), int(bad.size), host[bad[0]].tolist(), dev[bad[0]].tolist())
        # the host definition against Python's integers, for every case that is a field value: r 2^261 == a b + c d + e 2^261 (mod p), r below the
        # declared bound, limbs exact
        for (a, b, c, d, v), r in zip(cases, host):
            if not v:
                continue
            t = value(a) * value(a if form in SQR else b)
            if form in TWO:
                t += value(c) * value(d)
            if form in ADDHI:
                t += value(d) << 261
            got = value(r)
            assert (got << 261) % p == t % p and got < v * p and all(int(x) <= M29 for x in r), (field, form, a, b, c, d, r.tolist())


@pytest.mark.parametrize("field", ("fq", "fr"))
def test_wide_chains_of_256_operands_device_equals_host(gpu, host_twin, field):
    """lane i carries operand i through 255 in-place steps with the operands after it (x y, x^2 + y, y x + x y, x y + y in turn): 256 lanes, four waves"""
    p = MOD[field]
    rng = np.random.default_rng(7)
    vals = [0, p - 1, p, 5 * p, 6 * p - 1, (1 << 256) - 1] + [int.from_bytes(rng.bytes(32), "little") for _ in range(250)]
    ac = np.zeros((256, 18), dtype=np.uint32)
    ac[:, :9] = np.array([exact(v) for v in vals], dtype=np.uint32)
    bd = np.zeros_like(ac)
    host = host_twin(field, "wide_chain", ac, bd)
    dev = gpu.selftest_field_raw(field, "wide_chain", ac, bd)
    assert np.array_equal(host, dev), (field, int(np.nonzero((host != dev).any(axis=1))[0][0]))
    # lane 0 once more with Python's integers (residues only: the representative is the host's business)
    rinv = pow(1 << 261, -1, p)
    x = vals[0]
    for k in range(255):
        y = vals[(k + 1) % 256]
        x = (x * y * rinv, x * x * rinv + y, 2 * x * y * rinv, x * y * rinv + y)[k & 3] % p
    assert value(host[0]) % p == x and value(host[0]) < 9 * p


def test_madd_ip_representatives_inside_a_wave(gpu, oracle, ip_points):
    """one launch of 16 waves: in every wave lanes 0, 1, 2, 31, 32, 33 and 63 hold P + P, P - P, inf + Q, P - (-P), P + (-P), inf - Q and P + P on a
    fresh random representative (X l^2, Y l^3, Z l) of the accumulator -- so that P = x2 ZZ1 - X1 is a different multiple of p in each and its lazily
    reduced square lands on each of 0, p and 2 p -- while the other 57 lanes add two different points"""
    jac, aff, neg, dbl = ip_points
    m = len(jac)
    rng = np.random.default_rng(20261019)
    special = {0: 0, 1: 1, 2: 2, 31: 3, 32: 4, 33: 5, 63: 0}
    p_in, q_in, want = [], [], []
    for wave in range(16):
        for lane in range(64):
            i = (lane + wave) % m
            rep = representative(jac[i], int.from_bytes(rng.bytes(32), "little") % (FQ_MODULUS - 1) + 1)
            kind = special.get(lane)
            if kind == 0:
                p_in.append(rep); q_in.append(row(aff[i], False)); want.append(dbl[i])
            elif kind == 1:
                p_in.append(rep); q_in.append(row(aff[i], True)); want.append(inf_point())
            elif kind == 2:
                p_in.append(inf_point()); q_in.append(row(aff[i], False)); want.append(aff[i])
            elif kind == 3:
                p_in.append(rep); q_in.append(row(neg[i], True)); want.append(dbl[i])
            elif kind == 4:
                p_in.append(rep); q_in.append(row(neg[i], False)); want.append(inf_point())
            elif kind == 5:
                p_in.append(inf_point()); q_in.append(row(aff[i], True)); want.append(neg[i])
            else:
                k, s = (i + 1 + lane % (m - 1)) % m, lane % 3 == 0
                if k == i:
                    k = (i + 1) % m
                p_in.append(rep); q_in.append(row(aff[k], s))
                want.append(oracle.g1_normalize(oracle.g1_mixed_add(jac[i], (neg[k] if s else aff[k])[:8])))
    out = gpu.selftest_g1("madd_ip", np.stack(p_in), np.stack(q_in))
    for at, (r, w) in enumerate(zip(out, want)):
        assert np.array_equal(norm_xyzz(oracle, r), w), (at // 64, at % 64)


def test_msm_2e10_with_and_without_window_tables_equals_host_bucket_code(gpu, oracle):
    n = 1 << 10
    x = oracle.random_scalars(SRS_SEED, 1)[0]
    table = oracle.point_table(oracle.make_srs(x, n))
    scalars = oracle.random_scalars(SCALAR_SEED + 1019, n)
    want = gpu.host_msm(scalars, table, n)
    assert not int(want[7]) >> 63
    for precompute in (True, False):
        tab = aligned_copy(table)  # an address of its own: registered on first sight in the mode set now
        gpu.set_precompute(precompute)
        try:
            got = gpu.pippenger(scalars, tab, n)
            h = gpu.srs_register(tab)
            try:
                assert gpu.srs_has_window_tables(h) == precompute
            finally:
                gpu.srs_release(h)
        finally:
            gpu.set_precompute(True)
        assert np.array_equal(got[:8], want[:8]), "window tables" if precompute else "per-window bucket sets"


@pytest.mark.parametrize("log2n", (4, 10, 11))
def test_transforms_all_kinds_lifted_inputs(gpu, oracle, log2n):
    n = 1 << log2n
    const = oracle.random_scalars(CONST_SEED, 1)[0]
    co = canonical_residues(oracle, NTT_SEED + 2000 + log2n, n)
    classes = [c for c in input_classes(co) if c[0] != "canonical"]
    assert [c[0] for c in classes] == ["[0, 2r)", "max lift"]
    for kind in NTT_KINDS:
        want = oracle.ntt(co, kind, const)
        for cls, inp in classes:
            check_equal(gpu.ntt(inp.copy(), kind, const), want, "2^%d %s, %s input" % (log2n, kind, cls))
