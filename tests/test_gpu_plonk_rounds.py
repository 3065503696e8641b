"""The prover's round kernels (csrc/poly.hip) one at a time through bbgpu_selftest_plonk_round, against the plain statements of
tests/plonk_round_cases.py (pinned by tests/test_plonk_round_refs_host.py): every output of every lane, bit for bit -- the kernels store canonical values
and the arithmetic is exact, so there is no tolerance anywhere.

What whole proofs of the golden circuits never feed these kernels, and every case here does: selectors that are full-width field elements, q_c and q_bo
among them; operands over the whole admitted range (every second vector holds only the largest representatives below 2^256, and every lane of every
vector the raw values 0, r - 1, r, 2r, 5r and 2^256 - 1); lanes whose data and challenges all differ, with challenges 0 and r - 1 among them; and the
grid-stride kernels at 2^21 elements, where the 1024-workgroup cap makes every thread walk eight elements by x = x * step."""
import numpy as np
import pytest

from oracle.pyoracle import PolyOracle
from tests import plonk_round_cases as cases
from tests.plonk_round_cases import R

pytestmark = pytest.mark.gpu

LANES = (1, 2, 16)
MASKED = (8, 128, 256, 512, 4096)        # the kernel's own length: 2n (4n for the MiMC kernel); 8 is the n = 4 circuit, where every + 4 wraps
UNMASKED = (1, 255, 256, 257, 1000)
STRIDED = (16, 128, 1024, 2048, 8192)
BIG = 1 << 21                            # strided_blocks() caps the grid at 1024 workgroups of 256: eight elements per thread
SCAN_LENGTHS = (1, 8, 9, 2047, 2048, 2049, 5000)
COUNTS = (1, 3, 16)
UNWRITTEN = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def gpu():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.shutdown()


def plain_lanes(a, lanes):
    """[lane][i] plain residues of a lane-major array"""
    p = PolyOracle.plain(a)
    per = len(p) // lanes
    return [p[l * per:(l + 1) * per] for l in range(lanes)]


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero((got != want).any(axis=1))
    raise AssertionError("%s: %d of %d elements differ, the first at %d: got %s, want %s"
                         % (what, bad.size, got.shape[0], bad[0], [hex(int(v)) for v in got[bad[0]]], [hex(int(v)) for v in want[bad[0]]]))


def same_lanes(got, want_lanes, what):
    same(got, PolyOracle.mont([v for lane in want_lanes for v in lane]), what)


def seed_of(*parts):
    s = 0x706C6F6E6B
    for p in parts:
        s = (s * 0x100000001B3 + int(p)) & 0xFFFFFFFFFFFF
    return s


def big_indices(n, seed):
    """the indices checked where the vector is too long to restate in full: both ends, both sides of every multiple of the grid's 2^18 threads (where a
    thread takes its next step), and 4096 drawn ones"""
    nt = 262144
    idx = set(range(8)) | {k * nt + d for k in range(1, 8) for d in (-1, 0, 1)} | set(range(n - 5, n))
    idx |= {int(i) for i in np.random.default_rng(seed).integers(0, n, 4096)}
    assert all(0 <= i < n for i in idx)
    return sorted(idx)


def all_written(a):
    return not (np.asarray(a).reshape(-1, 4) == UNWRITTEN).all(axis=1).any()


# ---- grid-stride kernels -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", STRIDED)
@pytest.mark.parametrize("lanes", LANES)
def test_z_terms(gpu, oracle, lanes, n):
    vs = cases.input_vectors(oracle, seed_of(0, lanes, n), 6, lanes, n)
    ch, chm = cases.challenges(oracle, seed_of(0, lanes, n), lanes, 2)
    num, den = gpu.selftest_plonk_round("z_terms", lanes, n, vs, consts=chm)
    P = [plain_lanes(v, lanes) for v in vs]
    want = [cases.z_terms(*[p[l] for p in P], *ch[l], n) for l in range(lanes)]
    same_lanes(num, [w[0] for w in want], "num")
    same_lanes(den, [w[1] for w in want], "den")


@pytest.mark.parametrize("n4", STRIDED)
@pytest.mark.parametrize("lanes", LANES)
def test_quotient_large(gpu, oracle, lanes, n4):
    vs = cases.input_vectors(oracle, seed_of(1, lanes, n4), 7, lanes, n4)
    ch, chm = cases.challenges(oracle, seed_of(1, lanes, n4), lanes, 2)
    q, = gpu.selftest_plonk_round("quot_large", lanes, n4, vs, consts=chm)
    P = [plain_lanes(v, lanes) for v in vs]
    same_lanes(q, [cases.quot_large(*[p[l] for p in P], *ch[l], n4) for l in range(lanes)], "q")


@pytest.mark.parametrize("log2_ratio", (1, 2))
@pytest.mark.parametrize("N", STRIDED)
@pytest.mark.parametrize("lanes", LANES)
def test_divide_by_pseudo_vanishing(gpu, oracle, lanes, N, log2_ratio):
    """in place on lanes that lie `stride` > N elements apart: what lies between them stays as it was, word for word"""
    stride = N + 3
    c, = cases.input_vectors(oracle, seed_of(2, lanes, N, log2_ratio), 1, lanes, stride)
    got, = gpu.selftest_plonk_round("divide_vanishing", lanes, N, [c], params=(log2_ratio, stride))
    want = c.copy().reshape(lanes, stride, 4)
    for l in range(lanes):
        want[l, :N] = PolyOracle.divide_by_pseudo_vanishing(c.reshape(lanes, stride, 4)[l, :N], N >> log2_ratio, N)
    same(got, want, "coefficients")


def test_z_terms_eight_elements_per_thread(gpu, oracle):
    n = BIG
    vs = cases.input_vectors(oracle, seed_of(3), 6, 1, n)
    ch, chm = cases.challenges(oracle, seed_of(3), 1, 2)
    num, den = gpu.selftest_plonk_round("z_terms", 1, n, vs, consts=chm)
    assert all_written(num) and all_written(den)
    idx = big_indices(n, seed_of(3))
    wn, wd = cases.z_terms(*[cases.Rows(v) for v in vs], *ch[0], n, idx)
    same(num[idx], PolyOracle.mont(wn), "num")
    same(den[idx], PolyOracle.mont(wd), "den")


def test_quotient_large_eight_elements_per_thread(gpu, oracle):
    n4 = BIG
    vs = cases.input_vectors(oracle, seed_of(4), 7, 1, n4)
    ch, chm = cases.challenges(oracle, seed_of(4), 1, 2)
    q, = gpu.selftest_plonk_round("quot_large", 1, n4, vs, consts=chm)
    assert all_written(q)
    idx = big_indices(n4, seed_of(4))
    same(q[idx], PolyOracle.mont(cases.quot_large(*[cases.Rows(v) for v in vs], *ch[0], n4, idx)), "q")


def test_divide_by_pseudo_vanishing_eight_elements_per_thread(gpu, oracle):
    N, stride = BIG, BIG + 3
    c, = cases.input_vectors(oracle, seed_of(5), 1, 1, stride)
    got, = gpu.selftest_plonk_round("divide_vanishing", 1, N, [c], params=(2, stride))
    idx = big_indices(N, seed_of(5))
    same(got[idx], PolyOracle.mont(cases.divide_vanishing(cases.Rows(c), N >> 2, N, idx)), "coefficients")
    same(got[N:], c[N:], "behind the vector")


# ---- masked pointwise kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n2", MASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_quotient_mid(gpu, oracle, lanes, n2):
    """every selector a full-width field element, q_c (the one term behind the unrepaired constant) among them"""
    vs = cases.input_vectors(oracle, seed_of(6, lanes, n2), 10, lanes, [2 * n2] * 4 + [n2] * 6)
    ch, chm = cases.challenges(oracle, seed_of(6, lanes, n2), lanes, 2)
    q, = gpu.selftest_plonk_round("quot_mid", lanes, n2, vs, consts=chm)
    P = [plain_lanes(v, lanes) for v in vs]
    same_lanes(q, [cases.quot_mid(*[p[l] for p in P], *ch[l], n2) for l in range(lanes)], "q")


@pytest.mark.parametrize("n2", MASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_quotient_seq(gpu, oracle, lanes, n2):
    vs = cases.input_vectors(oracle, seed_of(7, lanes, n2), 3, lanes, [2 * n2, n2, n2])
    ch, chm = cases.challenges(oracle, seed_of(7, lanes, n2), lanes, 1)
    q, = gpu.selftest_plonk_round("quot_seq", lanes, n2, vs, consts=chm)
    pwo, pqon, pq = (plain_lanes(v, lanes) for v in vs)
    same_lanes(q, [cases.quot_seq(pq[l], pwo[l], pqon[l], ch[l][0], n2) for l in range(lanes)], "q")


@pytest.mark.parametrize("n2", MASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_quotient_bool(gpu, oracle, lanes, n2):
    """q_bl, q_br and q_bo full-width and live everywhere, on wires that are no booleans"""
    vs = cases.input_vectors(oracle, seed_of(8, lanes, n2), 7, lanes, [2 * n2] * 3 + [n2] * 4)
    ch, chm = cases.challenges(oracle, seed_of(8, lanes, n2), lanes, 3)
    q, = gpu.selftest_plonk_round("quot_bool", lanes, n2, vs, consts=chm)
    P = [plain_lanes(v, lanes) for v in vs]
    same_lanes(q, [cases.quot_bool(P[6][l], *[p[l] for p in P[:6]], *ch[l], n2) for l in range(lanes)], "q")


@pytest.mark.parametrize("n4", MASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_quotient_mimc(gpu, oracle, lanes, n4):
    vs = cases.input_vectors(oracle, seed_of(9, lanes, n4), 6, lanes, n4)
    ch, chm = cases.challenges(oracle, seed_of(9, lanes, n4), lanes, 2)
    q, = gpu.selftest_plonk_round("quot_mimc", lanes, n4, vs, consts=chm)
    P = [plain_lanes(v, lanes) for v in vs]
    same_lanes(q, [cases.quot_mimc(P[5][l], *[p[l] for p in P[:5]], *ch[l], n4) for l in range(lanes)], "q")


# ---- unmasked pointwise kernels ------------------------------------------------------------------------------------------------------------------------
def _lincomb(gpu, oracle, lanes, n, count, addend):
    vs = cases.input_vectors(oracle, seed_of(10, lanes, n, count, addend), count + addend, lanes, n)
    ch, chm = cases.challenges(oracle, seed_of(10, lanes, n, count, addend), lanes, count)
    out, = gpu.selftest_plonk_round("lincomb", lanes, n, vs, consts=chm, params=(count, addend))
    P = [plain_lanes(v, lanes) for v in vs]
    same_lanes(out, [cases.lincomb([p[l] for p in P[:count]], ch[l], P[count][l] if addend else None) for l in range(lanes)],
               "lincomb of %d%s" % (count, " with an addend" if addend else ""))


@pytest.mark.parametrize("n", UNMASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_lincomb(gpu, oracle, lanes, n):
    _lincomb(gpu, oracle, lanes, n, 12, 1)
    _lincomb(gpu, oracle, lanes, n, 7, 0)  # the linearisation polynomial's seven terms (prover.cpp:520-528)


@pytest.mark.parametrize("count", range(1, 13))
def test_lincomb_every_count(gpu, oracle, count):
    for addend in (0, 1):
        _lincomb(gpu, oracle, 2, 257, count, addend)


@pytest.mark.parametrize("n", UNMASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_mul2c(gpu, oracle, lanes, n):
    vs = cases.input_vectors(oracle, seed_of(11, lanes, n), 2, lanes, n)
    ch, chm = cases.challenges(oracle, seed_of(11, lanes, n), lanes, 1)
    out, = gpu.selftest_plonk_round("mul2c", lanes, n, vs, consts=chm)
    a, b = (plain_lanes(v, lanes) for v in vs)
    same_lanes(out, [cases.mul2c(a[l], b[l], ch[l][0]) for l in range(lanes)], "out")


@pytest.mark.parametrize("pad", (1, 4))
@pytest.mark.parametrize("n", UNMASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_sigma_prepare(gpu, oracle, lanes, n, pad):
    vs = cases.input_vectors(oracle, seed_of(12, lanes, n, pad), 2, lanes, n)
    ch, chm = cases.challenges(oracle, seed_of(12, lanes, n, pad), lanes, 1)
    dst, = gpu.selftest_plonk_round("sigma_prepare", lanes, n, vs, consts=chm, params=(pad * n,))
    s, w = (plain_lanes(v, lanes) for v in vs)
    same_lanes(dst, [cases.sigma_prepare(s[l], w[l], ch[l][0], pad * n) for l in range(lanes)], "dst")


@pytest.mark.parametrize("pad", (1, 4))
@pytest.mark.parametrize("n", UNMASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_copy_pad(gpu, oracle, lanes, n, pad):
    """scaled: c * src, canonical; plain: `src itself` (poly.h), the words as they are -- it moves a vector, and every consumer takes any representative"""
    src, = cases.input_vectors(oracle, seed_of(13, lanes, n, pad), 1, lanes, n)
    ch, chm = cases.challenges(oracle, seed_of(13, lanes, n, pad), lanes, 1)
    dst, = gpu.selftest_plonk_round("copy_pad", lanes, n, [src], consts=chm, params=(pad * n, 1))
    p = plain_lanes(src, lanes)
    same_lanes(dst, [cases.copy_pad_scaled(p[l], ch[l][0], pad * n) for l in range(lanes)], "scaled")
    dst, = gpu.selftest_plonk_round("copy_pad", lanes, n, [src], params=(pad * n, 0))
    want = np.zeros((lanes, pad * n, 4), dtype=np.uint64)
    want[:, :n] = src.reshape(lanes, n, 4)
    same(dst, want, "plain")


@pytest.mark.parametrize("n", UNMASKED)
@pytest.mark.parametrize("lanes", LANES)
def test_add_inplace(gpu, oracle, lanes, n):
    """quotient_mid (stride 2n) into quotient_large (stride 4n), prover.cpp:461-463: strides beyond n, and nothing behind n is touched"""
    sa, sb = 2 * n + 1, n + 3
    a, b = cases.input_vectors(oracle, seed_of(14, lanes, n), 2, lanes, [sa, sb])
    got, = gpu.selftest_plonk_round("add_inplace", lanes, n, [a, b], params=(sa, sb))
    want = a.copy().reshape(lanes, sa, 4)
    pa, pb = plain_lanes(a, lanes), plain_lanes(b, lanes)
    for l in range(lanes):
        want[l, :n] = PolyOracle.mont(cases.add_vectors(pa[l][:n], pb[l][:n]))
    same(got, want, "a")


# ---- scans and evaluations over a table of jobs ----------------------------------------------------------------------------------------------------------
def _scan_inputs(oracle, mode, n, count):
    v, = cases.input_vectors(oracle, seed_of(15, mode, n, count), 1, count, n)
    if mode == 0:
        # four of the six extremes are zero residues and would turn every product behind them into zero: the even jobs hold the next representative instead
        # (1, r + 1, 2r + 1, 5r + 1), the odd ones keep the zeros
        even = v.reshape(count, n, 4)[0::2]  # a view: the assignment below lands in v
        for val in (0, R, 2 * R, 5 * R):
            even[(even == cases.raw_rows([val])[0]).all(axis=2)] = cases.raw_rows([val + 1])[0]
    return v


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SCAN_LENGTHS)
@pytest.mark.parametrize("mode", (0, 1))
def test_scan_jobs(gpu, oracle, mode, n, count):
    """mode 0: running products, prefix or suffix (reverse); mode 1: Horner suffix sums in z, one z per job -- always a suffix scan, whatever `reverse` says
    (poly.hip).  Every reverse / inclusive combination, with an output vector, with vector and total, and for the total alone."""
    v = _scan_inputs(oracle, mode, n, count)
    ch, chm = cases.challenges(oracle, seed_of(15, mode, n, count), count, 1)
    p = plain_lanes(v, count)
    totals = [cases.product_of(p[j]) if mode == 0 else cases.evaluate(p[j], ch[j][0]) for j in range(count)]
    for inclusive in (0, 1):
        for reverse in (0, 1):
            if mode == 0:
                want = np.concatenate([PolyOracle.product_scan(v.reshape(count, n, 4)[j], bool(reverse), bool(inclusive)) for j in range(count)])
            elif reverse == 0:
                want = PolyOracle.mont([x for j in range(count) for x in cases.horner_suffix(p[j], ch[j][0], bool(inclusive))])
            for outputs in (4, 12, 8):
                flags = reverse | inclusive << 1 | outputs
                got = gpu.selftest_plonk_round("scan", count, n, [v], consts=chm if mode else None, params=(mode, flags))
                assert len(got) == (2 if outputs == 12 else 1)
                if outputs & 4:
                    same(got[0], want, "scan, flags %d" % flags)
                if outputs & 8:
                    same(got[-1], PolyOracle.mont(totals), "totals, flags %d" % flags)


@pytest.mark.parametrize("mode", (0, 1))
def test_scan_jobs_past_the_fused_form(gpu, oracle, mode):
    """2^19 + 1 elements leave 257 block totals per job, one more than the carry pass scans for itself: the totals get a level of their own, one
    workgroup per job, and the last block holds one element.  Two jobs (the entry takes 2^22 elements), vector and total: suffix products without the
    element itself, and inclusive Horner sums."""
    n, count = (1 << 19) + 1, 2
    v = _scan_inputs(oracle, mode, n, count)
    ch, chm = cases.challenges(oracle, seed_of(19, mode), count, 1)
    p = plain_lanes(v, count)
    if mode == 0:
        flags = 1 | 12
        want = np.concatenate([PolyOracle.product_scan(v.reshape(count, n, 4)[j], True, False) for j in range(count)])
        totals = [cases.product_of(p[j]) for j in range(count)]
    else:
        flags = 2 | 12
        sums = [cases.horner_suffix(p[j], ch[j][0], True) for j in range(count)]
        want = PolyOracle.mont([x for s in sums for x in s])
        totals = [cases.evaluate(p[j], ch[j][0]) for j in range(count)]
    got = gpu.selftest_plonk_round("scan", count, n, [v], consts=chm if mode else None, params=(mode, flags))
    assert len(got) == 2
    same(got[0], want, "scan, mode %d" % mode)
    same(got[1], PolyOracle.mont(totals), "totals, mode %d" % mode)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SCAN_LENGTHS)
def test_evaluate_jobs(gpu, oracle, n, count):
    """`count` polynomials at two points, the jobs picking theirs in no regular order; then at the points 0 and r - 1"""
    v, = cases.input_vectors(oracle, seed_of(16, n, count), 1, count, n)
    p = plain_lanes(v, count)
    zidx = [(j * j + j // 3 + 1) % 2 for j in range(count)]
    assert count == 1 or len(set(zidx)) == 2
    random_points = PolyOracle.plain(oracle.random_scalars(seed_of(17, n, count), 2))
    for points in (random_points, [0, R - 1]):
        got, = gpu.selftest_plonk_round("evaluate", count, n, [v], consts=PolyOracle.mont(points), params=[2] + zidx)
        same(got, PolyOracle.mont([cases.evaluate(p[j], points[zidx[j]]) for j in range(count)]), "evaluations at %s" % (points,))


# ---- what the entry refuses ----------------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_what_the_kernels_do_not_support(gpu, oracle):
    from barretenberg_amd.bbgpu import BbGpuError
    z = np.zeros((1 << 10, 4), dtype=np.uint64)
    for kernel, lanes, length, nin, consts, params in cases.REFUSED:
        with pytest.raises(BbGpuError, match="error -3"):
            gpu.selftest_plonk_round(kernel, lanes, length, [z] * nin, consts=consts, params=params)
    # and a call it takes still runs afterwards
    a, b = cases.input_vectors(oracle, seed_of(18), 2, 1, 8)
    ch, chm = cases.challenges(oracle, seed_of(18), 1, 1)
    out, = gpu.selftest_plonk_round("mul2c", 1, 8, [a, b], consts=chm)
    same(out, PolyOracle.mont(cases.mul2c(PolyOracle.plain(a), PolyOracle.plain(b), ch[0][0])), "out")
