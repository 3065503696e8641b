"""bbgpu_host_fr_fold / bbgpu_host_kate_opening_lagrange_folded (csrc/host_lagrange_open.hpp) and bbgpu_host_kzg_check_openings (csrc/host_kzg_check.hpp):
the definitions the opening sessions of the GPU are compared with bit for bit (tests/test_gpu_opening_session.py), and the argument verdicts of the new
device entries on a machine without a GPU.  CPU tests.  Expected values are the oracle's (tests/opening_session_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import FQ, FR, aligned_copy, from_int
from tests.lagrange_open_cases import ERR_ARG, ERR_SIZE, PAD, values, z_cases
from tests.opening_session_cases import ERR_STATE, add, fold, folded_expected, gamma_sets  # noqa: F401

SIZES = [2, 4, 8, 64, 256]


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("batch,pad", [(1, 0), (3, 0), (3, 5)])
def test_twins_against_the_definition(lib, oracle, n, batch, pad):
    """the fold and the folded opening at every kind of z (on and off the domain) and every kind of gamma; the values are read only"""
    stride = n + pad
    v = values(oracle, 0xF01D + n + batch, n, batch, stride)
    kept = v.copy()
    gammas = gamma_sets(oracle, batch)
    for gname, g in gammas:
        assert np.array_equal(lib.host_fold(v, g, n=n, stride=stride), fold(v, n, batch, stride, g)), gname
    for k, (name, z, _) in enumerate(z_cases(oracle, n)):
        gname, g = gammas[k % len(gammas)]
        f_want, q_want = folded_expected(oracle, v, n, batch, stride, g, z)
        q, f = lib.host_kate_opening_lagrange_folded(v, g, z, n=n, stride=stride)
        assert np.array_equal(f, f_want) and np.array_equal(q, q_want), (name, gname)
    assert np.array_equal(v, kept)


@pytest.mark.parametrize("n", SIZES)
def test_accumulate_over_two_calls_of_different_strides(lib, oracle, n):
    """two buffers (batch 2 at stride n + 5, batch 1 at stride n) folded into one vector and one quotient; F(z) is that of each call alone"""
    va, vb = values(oracle, 0xACC + n, n, 2, n + 5), values(oracle, 0xACD + n, n, 1, n)
    ga, gb = gamma_sets(oracle, 2)[0][1], gamma_sets(oracle, 1)[3][1]
    want_fold = add(fold(va, n, 2, n + 5, ga), fold(vb, n, 1, n, gb))
    out = lib.host_fold(va, ga, n=n, stride=n + 5)
    assert lib.host_fold(vb, gb, n=n, stride=n, out=out) is out and np.array_equal(out, want_fold)
    cases = z_cases(oracle, n)
    for name, z, _ in (cases[0], cases[3], cases[-1]):  # off the domain, at one, at w^(n/2 + 1)
        fa, qa = folded_expected(oracle, va, n, 2, n + 5, ga, z)
        fb, qb = folded_expected(oracle, vb, n, 1, n, gb, z)
        q, f = lib.host_kate_opening_lagrange_folded(va, ga, z, n=n, stride=n + 5)
        q2, f2 = lib.host_kate_opening_lagrange_folded(vb, gb, z, n=n, stride=n, out=q)
        assert q2 is q and np.array_equal(f, fa) and np.array_equal(f2, fb) and np.array_equal(q, add(qa, qb)), name
        lifted = q.copy()  # an accumulator that is not canonical comes out canonical
        lifted[:] = from_int((1 << 256) - 1)
        want = add(lifted, qb)
        lib.host_kate_opening_lagrange_folded(vb, gb, z, n=n, stride=n, out=lifted)
        assert np.array_equal(lifted, want), name


def test_twin_arguments(lib, oracle):
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import _ptr, u64p
    n = 8
    v, g, z = values(oracle, 1, n, 2, n), gamma_sets(oracle, 2)[0][1], oracle.random_scalars(2, 1)[0]
    for kw in (dict(n=0), dict(n=(1 << 24) + 1, stride=(1 << 24) + 1), dict(n=n, batch=0), dict(n=n, batch=65), dict(n=n, batch=2, stride=n - 1)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.host_fold(v, g, **dict(dict(batch=2, stride=n), **kw))
    assert np.array_equal(lib.host_fold(v[:6], g[:1], n=3, stride=3), fold(v, 3, 1, 3, g[:1]))  # the fold takes any length
    for kw in (dict(n=0), dict(n=1), dict(n=3), dict(n=1 << 25, stride=1 << 25), dict(n=n, batch=0), dict(n=n, batch=65), dict(n=n, batch=2, stride=n - 1)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.host_kate_opening_lagrange_folded(v, g, z, **dict(dict(batch=2, stride=n), **kw))
    L = lib.lib
    L.bbgpu_host_fr_fold.argtypes = [u64p, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, C.c_int]
    L.bbgpu_host_kate_opening_lagrange_folded.argtypes = [u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, u64p, C.c_int, u64p]
    out, f = np.zeros((n, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    for args in ((None, _ptr(v), n, n, 2, _ptr(g), 0), (_ptr(out), None, n, n, 2, _ptr(g), 0), (_ptr(out), _ptr(v), n, n, 2, None, 0)):
        assert L.bbgpu_host_fr_fold(*args) == -3
    for args in ((None, n, n, 2, _ptr(g), _ptr(z), _ptr(out), 0, _ptr(f)), (_ptr(v), n, n, 2, None, _ptr(z), _ptr(out), 0, _ptr(f)),
                 (_ptr(v), n, n, 2, _ptr(g), None, _ptr(out), 0, _ptr(f)), (_ptr(v), n, n, 2, _ptr(g), _ptr(z), None, 0, _ptr(f))):
        assert L.bbgpu_host_kate_opening_lagrange_folded(*args) == -3
    assert L.bbgpu_host_kate_opening_lagrange_folded(_ptr(v), n, n, 2, _ptr(g), _ptr(z), _ptr(out), 0, None) == 0  # folded_f_of_z may be NULL
    assert np.array_equal(out, lib.host_kate_opening_lagrange_folded(v, g, z, n=n, stride=n)[0])


def test_device_entries_refuse_their_arguments_before_a_device_is_bound(lib, oracle):
    """every argument error of every new device entry on a machine without a GPU: nothing is initialised for a call that is refused"""
    from barretenberg_amd import BbGpuError
    z, g = oracle.random_scalars(2, 4), gamma_sets(oracle, 2)[0][1]
    fake = 0x1000  # never dereferenced
    for kw in (dict(n=0), dict(n=1), dict(n=3), dict(n=1 << 25), dict(n=8, points=0), dict(n=8, points=5), dict(n=1 << 23, points=4), dict(n=1 << 24, points=2)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_begin(z=z, **kw)
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.lagrange_opening_begin(8, None, points=2)
    for batch in (0, 65):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_evaluate(0, 0, fake, 8, batch=batch)
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_open(0, 0, fake, fake, 8, batch=batch)
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.lagrange_opening_open_folded(0, 0, fake, 8, g, fake, batch=batch)
    for session in (-1, 0, 15, 16):  # no session exists
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_evaluate(session, 0, fake, 8)
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_open(session, 0, fake, fake, 8)
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_open_folded(session, 0, fake, 8, g, fake)
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.lagrange_opening_end(session)
    for call in (lambda: lib.lagrange_opening_evaluate(0, 0, None, 8), lambda: lib.lagrange_opening_open(0, 0, None, fake, 8),
                 lambda: lib.lagrange_opening_open(0, 0, fake, None, 8), lambda: lib.lagrange_opening_open_folded(0, 0, None, 8, g, fake),
                 lambda: lib.lagrange_opening_open_folded(0, 0, fake, 8, g, None), lambda: lib.lagrange_opening_open_folded(0, 0, fake, 8, None, fake, batch=2)):
        with pytest.raises(BbGpuError, match=ERR_ARG):
            call()
    for kw in (dict(n=0), dict(n=(1 << 24) + 1), dict(n=8, batch=0), dict(n=8, batch=65), dict(n=8, stride=7)):
        with pytest.raises(BbGpuError, match=ERR_SIZE):
            lib.fold_device(fake, fake, gamma=g, **kw)
    for args in ((None, fake, g), (fake, None, g), (fake, fake, None)):
        with pytest.raises(BbGpuError, match=ERR_ARG):
            lib.fold_device(args[0], args[1], 8, args[2], batch=2)


# ---- bbgpu_host_kzg_check_openings over a small string --------------------------------------------------------------------------------------------------
N = 16


@pytest.fixture(scope="module")
def string(lib, oracle, tmp_path_factory):
    """the Lagrange form of an honest string of 16 rows as a plain table, x G2, and five polynomials with their commitments"""
    from tests.srs_check_cases import g2_of
    from tests.srs_update_cases import honest_table, secret_x
    x = secret_x(oracle)
    lagrange, _ = lib.host_srs_lagrange(honest_table(oracle, x, N), N)
    rows = aligned_copy(lagrange[0::2])
    v = values(oracle, 0x4A7E, N, 5)
    commitments = np.stack([lib.host_msm(aligned_copy(v[b * N:(b + 1) * N]), rows, N, plain=True)[:8] for b in range(5)])
    return dict(rows=rows, g2_x=g2_of(lib, oracle, tmp_path_factory.mktemp("g2"), x, "x.dat"), v=v, commitments=commitments)


def claim(lib, S, polys, gamma, z):
    """(C, z, y, pi) of the folded opening of the polynomials `polys` at z"""
    v = aligned_copy(np.concatenate([S["v"][b * N:(b + 1) * N] for b in polys]))
    q, y = lib.host_kate_opening_lagrange_folded(v, gamma, z, n=N, stride=N)
    c = lib.host_msm(aligned_copy(gamma), aligned_copy(S["commitments"][list(polys)]), len(polys), plain=True)[:8]
    return c, np.array(z, dtype=np.uint64), y, lib.host_msm(q, S["rows"], N, plain=True)[:8]


def verdict(lib, S, claims, seed=None):
    return lib.host_kzg_check_openings(*[np.stack([c[k] for c in claims]) for k in range(4)], S["g2_x"], seed=seed)


def test_kzg_check(lib, oracle, string):
    from barretenberg_amd import BbGpuError
    from tests.srs_check_cases import SEED
    S = string
    cases = z_cases(oracle, N)
    z_off, z_on, z_w = cases[0][1], cases[-1][1], cases[5][1]
    g3, g2, g1 = gamma_sets(oracle, 3)[0][1], gamma_sets(oracle, 2)[3][1], gamma_sets(oracle, 1)[1][1]
    one = claim(lib, S, (0, 1, 2), g3, z_off)
    assert verdict(lib, S, [one], SEED) and verdict(lib, S, [one])  # k = 1; a caller's seed and the operating system's
    three = [one, claim(lib, S, (3, 4), g2, z_on), claim(lib, S, (2,), g1, z_w)]  # k = 3 at mixed points: off the domain, on it, on it with one polynomial
    assert verdict(lib, S, three, SEED) and verdict(lib, S, three)
    for t in range(3):  # a y + 1
        bad = [list(c) for c in three]
        bad[t][2] = oracle.add(FR, bad[t][2], oracle.const(FR, "one"))
        assert not verdict(lib, S, bad, SEED), t
    swapped = [list(c) for c in three]  # two exchanged proofs
    swapped[0][3], swapped[1][3] = three[1][3], three[0][3]
    assert not verdict(lib, S, swapped, SEED)
    other = [list(c) for c in three]  # a commitment folded with other multipliers
    other[0][0] = lib.host_msm(aligned_copy(gamma_sets(oracle, 3)[1][1]), aligned_copy(S["commitments"][[0, 1, 2]]), 3, plain=True)[:8]
    assert not verdict(lib, S, other, SEED)
    for k in (0, 3):  # a finite point off the curve, as a commitment and as a proof
        off_curve = [list(c) for c in three]
        off_curve[1][k] = off_curve[1][k].copy()
        off_curve[1][k][4:] = oracle.add(FQ, off_curve[1][k][4:], oracle.const(FQ, "one"))
        with pytest.raises(BbGpuError, match=ERR_ARG):
            verdict(lib, S, off_curve, SEED)
    # the infinity flag is honoured: the zero polynomial commits to infinity, its quotient too, and the claim 0 = 0 holds
    inf = np.zeros(8, dtype=np.uint64)
    inf[7] = 1 << 63
    assert verdict(lib, S, three + [(inf, z_off, from_int(0), inf)], SEED)
    assert not verdict(lib, S, three + [(inf, z_off, oracle.const(FR, "one"), inf)], SEED)
    bad_g2 = S["g2_x"].copy()
    bad_g2[0] ^= 1
    with pytest.raises(BbGpuError, match=ERR_ARG):
        lib.host_kzg_check_openings(*[np.stack([c[k] for c in three]) for k in range(4)], bad_g2, seed=SEED)
    with pytest.raises(BbGpuError, match=ERR_SIZE):
        lib.host_kzg_check_openings(np.zeros((65, 8), dtype=np.uint64), np.zeros((65, 4), dtype=np.uint64), np.zeros((65, 4), dtype=np.uint64),
                                    np.zeros((65, 8), dtype=np.uint64), S["g2_x"], seed=SEED)
    with pytest.raises(BbGpuError, match=ERR_SIZE):
        lib.host_kzg_check_openings(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64),
                                    np.zeros((0, 8), dtype=np.uint64), S["g2_x"], seed=SEED)


def test_host_twins_under_sanitizers(tmp_path):
    """tests/cpp/test_opening_session_host.cpp: the fold and the folded opening as a stand-alone program (own main) built with
    -fsanitize=address,undefined: n = 2 and 64, on and off the domain, with padding, with accumulate over two calls, against the unfolded twin"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "test_opening_session_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    os.path.join(root, "tests", "cpp", "test_opening_session_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout and "MISMATCH" not in r.stdout
