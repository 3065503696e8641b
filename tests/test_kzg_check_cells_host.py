"""bbgpu_host_kzg_check_cells / bbgpu_host_kzg_check_open_cosets / bbgpu_host_kzg_cells_key_check (csrc/host_kzg_check_cells.hpp): the definition the
GPU entries are compared with field for field (tests/test_gpu_kzg_check_cells.py), against an independent reference (tests/kzg_check_cells_cases.py:
Lagrange interpolation over Python integers, bbgpu_host_msm_g1, bbgpu_host_pairing_check), the two forms against each other, l = 1 against the open-all
check, every false claim, the key check, the findings and the argument verdicts of all five entries on a machine without a GPU.  CPU tests."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FR_MODULUS as R, aligned_copy, from_int, to_int
from tests.kzg_check_cells_cases import (ERR_ARG, ERR_SIZE, INF, SEED, SIZES, above_r, args_of, cells_of, cosets_args, cosets_as_labelled, honest, make_world,
                                         memory, negated, off_curve, padded, plus_one, power_of_secret, reference, scalars)
from tests.srs_check_cases import g2_of


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def worlds(lib, oracle, tmp_path_factory):
    """one world per (n, l, batch), made on first use, never written to"""
    made = {}

    def world(n, l, batch=3):
        if (n, l, batch) not in made:
            made[(n, l, batch)] = make_world(lib, oracle, tmp_path_factory.mktemp("cells_%d_%d_%d" % (n, l, batch)), n, l, batch)
        return made[(n, l, batch)]
    return world


def against_reference(lib, oracle, W, which, cell, values, proofs, **kw):
    """the twin's report with LOCATE; a, b, ok and first_failing are the reference's"""
    a = args_of(W, which, cell, values, proofs, **kw)
    got = lib.host_kzg_check_cells(*a, seed=SEED, locate=True)
    want = reference(lib, oracle, W, a[0], which, cell, values, proofs, a[7], a[8])
    assert {k: got[k] for k in want} == want, (got, want)
    return got


@pytest.mark.parametrize("n,l,batch,count", [(n, l, 2 + l % 2, 7) for n, l in SIZES] + [(256, 4, 3, 200), (128, 64, 2, 5)])
def test_twin_against_the_reference(lib, oracle, worlds, n, l, batch, count):
    """A, B and the verdict of the definition, cells of two or three commitments in scrambled order with duplicates; then one false value, located"""
    W = worlds(n, l, batch)
    which, cell, values, proofs = cells_of(W, count)
    assert count > batch * W["m"] or len({(int(b), int(k)) for b, k in zip(which, cell)}) == count
    got = against_reference(lib, oracle, W, which, cell, values, proofs)
    assert scalars(got) == honest(count) and got["seed"] == [int(v) for v in SEED]
    if count > 10:
        return  # the reference costs an interpolation and a pairing per cell: the tampers run at the small counts
    v2 = values.copy()
    t = count // 2
    v2[t * l + l - 1] = plus_one(oracle, v2[t * l + l - 1])
    got = against_reference(lib, oracle, W, which, cell, v2, proofs)
    assert got["ok"] == 0 and got["first_failing"] == t


def test_duplicates_and_many_cells(lib, oracle, worlds):
    """(8, 4): 2 cells per polynomial, 7 cells of 2 polynomials -- the same (label, cell) several times"""
    W = worlds(8, 4, 2)
    which, cell, values, proofs = cells_of(W, 7)
    assert len({(int(b), int(k)) for b, k in zip(which, cell)}) < 7
    assert scalars(against_reference(lib, oracle, W, which, cell, values, proofs)) == honest(7)


@pytest.mark.parametrize("n,batch", [(2, 1), (16, 3)])
def test_cosets_of_one_point_are_the_open_all_check(lib, oracle, worlds, n, batch):
    """l = 1 with P_0 = G and g2_xl = g2_x: the report of bbgpu_host_kzg_check_open_all, field for field"""
    W = worlds(n, 1, batch)
    assert np.array_equal(W["g2_xl"], W["g2_x"])
    got = lib.host_kzg_check_open_cosets(*cosets_args(W), seed=SEED)
    assert got == lib.host_kzg_check_open_all(W["commitments"], W["values"], W["proofs"], n, W["g2_x"], seed=SEED) and scalars(got) == honest(n * batch)
    values = aligned_copy(W["values"].reshape(-1, 4))
    values[n * batch - 2] = plus_one(oracle, values[n * batch - 2])
    got = lib.host_kzg_check_open_cosets(*cosets_args(W, values=values), seed=SEED, locate=True)
    assert got == lib.host_kzg_check_open_all(W["commitments"], values, W["proofs"], n, W["g2_x"], seed=SEED, locate=True) and got["first_failing"] == n * batch - 2


@pytest.mark.parametrize("n,l", [(8, 4), (16, 2), (128, 64)])
def test_the_proofs_of_open_cosets_are_accepted_in_both_forms(lib, oracle, worlds, n, l):
    """what bbgpu_host_kzg_open_cosets wrote: ok in the open-cosets form, padded and not, and the same report from the labelled form; the padding is not read"""
    W = worlds(n, l, 3)
    want = lib.host_kzg_check_cells(*args_of(W, *cosets_as_labelled(W)), seed=SEED)
    assert scalars(want) == honest(3 * W["m"])
    assert lib.host_kzg_check_open_cosets(*cosets_args(W), seed=SEED) == want
    buf, stride = padded(oracle, W, 5)
    assert lib.host_kzg_check_open_cosets(*cosets_args(W, values=buf), stride=stride, seed=SEED) == want
    buf[n:stride] = plus_one(oracle, buf[n])
    assert lib.host_kzg_check_open_cosets(*cosets_args(W, values=buf), stride=stride, seed=SEED) == want
    buf[2 * stride + n - 1] = plus_one(oracle, buf[2 * stride + n - 1])  # the last value of the last cell of the last polynomial
    got = lib.host_kzg_check_open_cosets(*cosets_args(W, values=buf), stride=stride, seed=SEED, locate=True)
    assert got["ok"] == 0 and got["first_failing"] == 3 * W["m"] - 1


@pytest.mark.parametrize("n,l", [(8, 4), (128, 64)])
def test_every_false_claim_is_rejected_and_located(lib, oracle, worlds, tmp_path, n, l):
    W = worlds(n, l, 3)
    count, t = 6, 4
    which, cell, values, proofs = cells_of(W, count)

    def located(**kw):
        a = dict(dict(which=which, cell=cell, values=values, proofs=proofs), **kw)
        extra = {k: a.pop(k) for k in ("g2_xl",) if k in a}
        got = lib.host_kzg_check_cells(*args_of(W, a["which"], a["cell"], a["values"], a["proofs"], **extra), seed=SEED, locate=True)
        assert got["ok"] == 0 and got["rounds"] >= 2, got
        assert lib.host_kzg_check_cells(*args_of(W, a["which"], a["cell"], a["values"], a["proofs"], **extra), seed=SEED)["first_failing"] == -1
        return got["first_failing"]

    for j in sorted({0, 1, l - 1}):  # one value + 1
        v2 = values.copy()
        v2[t * l + j] = plus_one(oracle, v2[t * l + j])
        assert located(values=v2) == t, j
    v2 = values.copy()  # two unequal values of a cell swapped
    assert not np.array_equal(v2[t * l], v2[t * l + 1])
    v2[[t * l, t * l + 1]] = v2[[t * l + 1, t * l]]
    assert located(values=v2) == t
    c2 = cell.copy()  # cell index k + 1
    c2[t] = (c2[t] + 1) % W["m"]
    assert located(cell=c2) == t
    w2 = which.copy()  # another label
    w2[t] = (w2[t] + 1) % 3
    assert located(which=w2) == t
    p2 = proofs.copy()  # the proof negated
    p2[t] = negated(oracle, p2[t])
    assert located(proofs=p2) == t
    p2 = proofs.copy()  # another cell's proof
    p2[t] = proofs[t - 1]
    assert not np.array_equal(proofs[t], proofs[t - 1])
    assert located(proofs=p2) == t
    g2_other = g2_of(lib, oracle, tmp_path, plus_one(oracle, power_of_secret(oracle, l)), "xl1.dat")  # the g2_xl of x^l + 1
    assert located(g2_xl=g2_other) == 0


@pytest.mark.parametrize("n,l", [(2, 1), (8, 4), (128, 64)])
def test_key_check(lib, oracle, worlds, tmp_path, n, l):
    W = worlds(n, l, 3 if (n, l) != (2, 1) else 1)
    assert lib.host_kzg_cells_key_check(W["head"], l, W["g2_x"], W["g2_xl"]) is True
    shifted = aligned_copy(W["table"][2:2 * l + 2:2])  # the head shifted by one row: P_1 .. P_l
    assert lib.host_kzg_cells_key_check(shifted, l, W["g2_x"], W["g2_xl"]) is False
    other = g2_of(lib, oracle, tmp_path, power_of_secret(oracle, l + 1), "other.dat")  # the g2_xl of another power
    assert lib.host_kzg_cells_key_check(W["head"], l, W["g2_x"], other) is False
    off = W["g2_xl"].copy()
    off[8:12] = from_int((to_int(off[8:12]) + 1) % (1 << 256))  # off the twist
    assert lib.host_kzg_cells_key_check(W["head"], l, W["g2_x"], off) is False
    bad_head = W["head"].copy()
    bad_head[l - 1] = off_curve(oracle, bad_head[l - 1])
    assert lib.host_kzg_cells_key_check(bad_head, l, W["g2_x"], W["g2_xl"]) is False


def test_points_off_the_curve_are_findings(lib, oracle, worlds):
    """a finite commitment or proof off the curve is counted and named, ok = 0, no sums are taken (a and b stay at infinity)"""
    W = worlds(8, 4, 3)
    which, cell, values, proofs = cells_of(W, 6)
    inf = [int(v) for v in INF]
    p2 = proofs.copy()
    p2[2], p2[5] = off_curve(oracle, proofs[2]), off_curve(oracle, proofs[5])
    rep = lib.host_kzg_check_cells(*args_of(W, which, cell, values, p2), seed=SEED, locate=True)
    assert scalars(rep) == honest(6, ok=0, rounds=0, bad_points=2, first_bad=2, first_bad_is_proof=1) and rep["a"] == inf and rep["b"] == inf
    sh = W["commitments"].copy()
    sh[1] = off_curve(oracle, sh[1])
    rep = lib.host_kzg_check_cells(*args_of(W, which, cell, values, p2, commitments=sh), seed=SEED)  # a shared commitment comes before every cell
    assert scalars(rep) == honest(6, ok=0, rounds=0, bad_points=3, first_bad=1, first_bad_is_proof=0)
    pr = W["proofs"].copy()
    pr[2, 1] = off_curve(oracle, pr[2, 1])
    rep = lib.host_kzg_check_open_cosets(*cosets_args(W, proofs=pr), seed=SEED)
    assert scalars(rep) == honest(6, ok=0, rounds=0, bad_points=1, first_bad=5, first_bad_is_proof=1)
    rep = lib.host_kzg_check_open_cosets(*cosets_args(W, proofs=pr, commitments=sh), seed=SEED)
    assert scalars(rep) == honest(6, ok=0, rounds=0, bad_points=2, first_bad=1, first_bad_is_proof=0)


def test_special_polynomials(lib, oracle, worlds, tmp_path):
    """degree < l (all proofs at infinity: A and B at infinity, ok), an all-zero cell, a constant cell, a commitment at infinity (the zero polynomial),
    values given as v + r"""
    n, l, m = 16, 4, 4
    rnd = oracle.random_scalars(0x5BEC, 3 * n).reshape(3, n, 4).copy()
    rnd[0, l:] = 0  # degree < l
    rnd[1] = 0      # the zero polynomial: its commitment is at infinity, every cell all zero
    rnd[2, 1:] = 0  # a constant: every cell constant
    W = make_world(lib, oracle, tmp_path, n, l, 3, coeffs=rnd)
    inf = [int(v) for v in INF]
    assert np.array_equal(W["proofs"], np.tile(INF, (3, m, 1))) and np.array_equal(W["commitments"][1], INF)
    assert not W["values"][1].any() and all(np.array_equal(W["values"][2, i], W["values"][2, 0]) for i in range(n))
    got = lib.host_kzg_check_open_cosets(*cosets_args(W), seed=SEED)
    assert scalars(got) == honest(3 * m) and got["a"] == inf and got["b"] == inf
    which, cell, values, proofs = cosets_as_labelled(W)
    assert scalars(against_reference(lib, oracle, W, which, cell, values, proofs)) == honest(3 * m)
    v2 = values.copy()
    v2[5 * l + 2] = plus_one(oracle, v2[5 * l + 2])  # an all-zero cell that is not
    assert against_reference(lib, oracle, W, which, cell, v2, proofs)["first_failing"] == 5
    # values as v + r where that fits in 256 bits: the same report
    V = worlds(8, 4, 3)
    which, cell, values, proofs = cells_of(V, 6)
    want = lib.host_kzg_check_cells(*args_of(V, which, cell, values, proofs), seed=SEED)
    v2 = values.copy()
    moved = 0
    for i in range(v2.shape[0]):
        if to_int(v2[i]) + R < (1 << 256):
            v2[i] = above_r(v2[i])
            moved += 1
    assert moved > 0 and lib.host_kzg_check_cells(*args_of(V, which, cell, v2, proofs), seed=SEED) == want and want["ok"] == 1


def test_a_seed_from_the_operating_system_is_reported(lib, worlds):
    W = worlds(8, 4, 3)
    a, b = lib.host_kzg_check_open_cosets(*cosets_args(W)), lib.host_kzg_check_open_cosets(*cosets_args(W))
    assert a["ok"] == b["ok"] == 1 and a["seed"] != b["seed"] and a["a"] != b["a"]
    assert lib.host_kzg_check_open_cosets(*cosets_args(W), seed=np.array(a["seed"], dtype=np.uint64)) == a  # a finding can be replayed


def test_argument_errors(lib, oracle, worlds):
    """every argument error of the five entries -- the device entries refuse before a device is bound, so a machine without a GPU gives the same verdicts"""
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import KzgCheckReport, _ptr, u64p
    W = worlds(8, 4, 3)
    n, l, m = 8, 4, 2
    which, cell, values, proofs = cells_of(W, 6)
    u32p = C.POINTER(C.c_uint32)
    rep = KzgCheckReport()
    seed = aligned_copy(SEED)
    g2 = W["g2_xl"]
    bad_g2 = g2.copy()
    bad_g2[0] ^= 1
    inf_g2 = g2.copy()
    inf_g2[15] |= np.uint64(1 << 63)
    head_off, head_inf = W["head"].copy(), W["head"].copy()
    head_off[2] = off_curve(oracle, head_off[2])
    head_inf[3] = INF
    keep = []

    def u32(w):
        keep.append(np.ascontiguousarray(w, dtype=np.uint32))
        return keep[-1].ctypes.data_as(u32p)

    def call(fn, good, **changes):
        a = list(good)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return fn(*a)

    for fn in (lib.lib.bbgpu_kzg_check_cells, lib.lib.bbgpu_host_kzg_check_cells):
        fn.argtypes = [u64p, C.c_size_t, u32p, u32p, u64p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        good = [_ptr(W["commitments"]), 3, u32(which), u32(cell), _ptr(values), _ptr(proofs), 6, n, l, _ptr(W["head"]), _ptr(g2), _ptr(seed), 0, C.byref(rep)]
        for coset in (0, 3, 128):
            assert call(fn, good, a8=coset) == -2, coset
        for nn in (0, 12, 4, 1 << 22):  # not a power of two; n / coset < 2; above 2^21
            assert call(fn, good, a7=nn) == -2, nn
        for count in (0, (1 << 20) + 1, (1 << 18) + 1):  # count outside 1 .. 2^20; count x coset above 2^20
            assert call(fn, good, a6=count) == -2, count
        for k in (0, 2, 3, 4, 5, 9, 10, 13):  # null commitments / which / cell / values / proofs / g1_head / g2_xl / report
            assert call(fn, good, **{"a%d" % k: None}) == -3, k
        for num in (0, 65, 2):  # outside 1 .. 64; a label out of range
            assert call(fn, good, a1=num) == -3, num
        assert call(fn, good, a3=u32([0, 1, 2, 0, 1, 0])) == -3  # a cell index out of range
        for flags in (2, 4, -1):
            assert call(fn, good, a12=flags) == -3
        for g in (bad_g2, inf_g2):
            assert call(fn, good, a10=_ptr(g)) == -3
        assert call(fn, good, a9=_ptr(head_off)) == -3 and b"row 2" in lib.lib.bbgpu_last_error() and b"off the curve" in lib.lib.bbgpu_last_error()
        assert call(fn, good, a9=_ptr(head_inf)) == -3 and b"row 3" in lib.lib.bbgpu_last_error() and b"infinity" in lib.lib.bbgpu_last_error()
        if fn is lib.lib.bbgpu_host_kzg_check_cells:  # the call itself is good (the device entry would go on to bind a device)
            assert call(fn, good) == 0 and rep.ok == 1
    for fn in (lib.lib.bbgpu_kzg_check_open_cosets, lib.lib.bbgpu_host_kzg_check_open_cosets):
        fn.argtypes = [u64p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        vals, prf = aligned_copy(W["values"].reshape(-1, 4)), aligned_copy(W["proofs"].reshape(-1, 8))
        good = [_ptr(W["commitments"]), _ptr(vals), n, _ptr(prf), n, l, 3, _ptr(W["head"]), _ptr(g2), _ptr(seed), 0, C.byref(rep)]
        for coset in (0, 3, 128, 8):  # 8: n / coset < 2
            assert call(fn, good, a5=coset) == -2, coset
        for nn in (0, 12, 1 << 22):
            assert call(fn, good, a4=nn, a2=max(nn, n)) == -2, nn
        for batch in (0, -1, 65):
            assert call(fn, good, a6=batch) == -2, batch
        assert call(fn, good, a2=n - 1) == -2  # stride < n
        assert call(fn, good, a4=1 << 15, a2=1 << 15, a6=33) == -2 and call(fn, good, a4=1 << 21, a2=1 << 21, a6=1) == -2  # batch x n above 2^20
        for k in (0, 1, 3, 7, 8, 11):
            assert call(fn, good, **{"a%d" % k: None}) == -3, k
        assert call(fn, good, a10=2) == -3 and call(fn, good, a8=_ptr(bad_g2)) == -3 and call(fn, good, a7=_ptr(head_off)) == -3
        if fn is lib.lib.bbgpu_host_kzg_check_open_cosets:
            assert call(fn, good) == 0 and rep.ok == 1 and rep.count == 3 * m
    fn = lib.lib.bbgpu_host_kzg_cells_key_check
    fn.argtypes = [u64p, C.c_size_t, u64p, u64p, C.POINTER(C.c_int)]
    ok = C.c_int(0)
    good = [_ptr(W["head"]), l, _ptr(W["g2_x"]), _ptr(g2), C.byref(ok)]
    for coset in (0, 3, 128):
        assert call(fn, good, a1=coset) == -2
    for k in (0, 2, 3, 4):
        assert call(fn, good, **{"a%d" % k: None}) == -3
    assert call(fn, good) == 0 and ok.value == 1
    # through the binding: the message names the entry's family
    with pytest.raises(BbGpuError, match=ERR_SIZE + " KZG check"):
        lib.kzg_check_open_cosets(*cosets_args(W)[:3], 0, *cosets_args(W)[4:], seed=SEED)
    with pytest.raises(BbGpuError, match=ERR_ARG + " KZG check"):
        lib.kzg_check_cells(*args_of(W, which, cell, values, proofs, g2_xl=bad_g2), seed=SEED)


def test_host_twin_under_sanitizers(tmp_path):
    """tests/cpp/test_kzg_check_cells_host.cpp: the twin as a stand-alone program (own main, nothing preloaded) built with -fsanitize=address,undefined:
    the two forms against each other and against the cell-by-cell definition at l = 4 and l = 64, infinities, findings, the key check, the bisection"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_kzg_check_cells_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_kzg_check_cells_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
