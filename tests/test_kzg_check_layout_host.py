"""bbgpu_host_kzg_check_cells_layout / bbgpu_host_kzg_check_open_cosets_layout (csrc/host_kzg_check_cells.hpp with the cap of 2^16 commitments): up to
64 commitments the reports of the twins of bbgpu_kzg_check_cells / bbgpu_kzg_check_open_cosets field for field; above, A, B and the verdict of the
independent reference of tests/kzg_check_cells_cases.py; a false commitment under a label >= 64 located; the argument verdicts of all four layout entries
-- the device entries refuse before a device is bound -- on a machine without a GPU.  CPU tests."""
import ctypes as C

import numpy as np
import pytest

import tests.kzg_check_cells_cases as cases
from oracle.pyoracle import aligned_copy
from tests.kzg_check_cells_cases import SEED, SIZES, args_of, cells_of, cosets_args, cosets_as_labelled, honest, padded, reference, scalars
from tests.kzg_check_layout_cases import MAX_S, cells_under, commitments_of, make_worlds, mixed, rows_world


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    return BbGpu(init=False)  # never binds a device


@pytest.fixture(scope="module")
def worlds(lib, oracle, tmp_path_factory):
    return make_worlds(lib, oracle, tmp_path_factory)


def test_cells_under_is_cells_of(worlds):
    """the fixture builder of these tests at labels t % 8 is tests.kzg_check_cells_cases.cells_of"""
    W = worlds(16, 4)
    for got, want in zip(cells_under(W, np.arange(5, 45) % 8, start=5), cells_of(W, 40, start=5)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("n,l", SIZES)
def test_up_to_64_commitments_the_reports_are_the_old_twins(lib, oracle, worlds, n, l):
    """both forms, S = 8 and S = 64, honest and with a false value under LOCATE: field for field under one seed"""
    W = worlds(n, l)
    for S in (8, 64):
        which, cell, values, proofs = cells_under(W, mixed(S, 40))
        a = args_of(W, which, cell, values, proofs, commitments=commitments_of(W, S))
        got = lib.host_kzg_check_cells_layout(*a, seed=SEED)
        assert got == lib.host_kzg_check_cells(*a, seed=SEED) and scalars(got) == honest(40), (S, got)
        v2 = values.copy()
        v2[13 * l + l - 1] = cases.plus_one(oracle, v2[13 * l + l - 1])
        a = args_of(W, which, cell, v2, proofs, commitments=commitments_of(W, S))
        got = lib.host_kzg_check_cells_layout(*a, seed=SEED, locate=True)
        assert got == lib.host_kzg_check_cells(*a, seed=SEED, locate=True) and got["ok"] == 0 and got["first_failing"] == 13, (S, got)
    V = rows_world(W, 11)
    buf, stride = padded(oracle, V, 3)
    for kw in (dict(), dict(values=buf)):
        st = stride if kw else None
        got = lib.host_kzg_check_open_cosets_layout(*cosets_args(V, **kw), stride=st, seed=SEED)
        assert got == lib.host_kzg_check_open_cosets(*cosets_args(V, **kw), stride=st, seed=SEED) and scalars(got) == honest(11 * W["m"]), got


@pytest.mark.parametrize("n,l", [(16, 4), (128, 64)])
@pytest.mark.parametrize("S", [65, 257])
def test_above_64_commitments_against_the_reference(lib, oracle, worlds, monkeypatch, n, l, S):
    """300 cells with mixed labels, duplicates, commitments that own no cell: ok, and A and B are the independent reference's.  The world has 8 x m distinct
    cells, so the reference's Lagrange interpolation is remembered by its arguments (the same naive function, called once per distinct cell)."""
    plain_interpolate, memo = cases.interpolate, {}

    def remembered(zs, vs):
        key = (tuple(zs), tuple(vs))
        if key not in memo:
            memo[key] = plain_interpolate(zs, vs)
        return memo[key]
    monkeypatch.setattr(cases, "interpolate", remembered)
    W = worlds(n, l)
    count = 300
    labels = mixed(S, count)
    assert labels.max() >= 64 and len(set(labels.tolist())) < min(S, count) and len(set(range(S)) - set(labels.tolist())) > 0
    which, cell, values, proofs = cells_under(W, labels)
    assert len({(int(c), int(k)) for c, k in zip(which, cell)}) < count  # duplicates
    cs = commitments_of(W, S)
    a = args_of(W, which, cell, values, proofs, commitments=cs)
    got = lib.host_kzg_check_cells_layout(*a, seed=SEED, locate=True)
    want = reference(lib, oracle, W, cs, which, cell, values, proofs, a[7], a[8])
    assert scalars(got) == honest(count) and {k: got[k] for k in want} == want, (got, want)


@pytest.mark.parametrize("n,l", [(16, 4), (128, 64)])
def test_a_false_commitment_above_label_64_is_located(lib, oracle, worlds, n, l):
    """commitment 201 of 257 replaced by another polynomial's: ok = 0, and with LOCATE first_failing is the first cell that carries label 201"""
    W = worlds(n, l)
    S, count, c = 257, 300, 201
    labels = mixed(S, count)
    t = int(np.flatnonzero(labels == c)[0])
    assert t > 0
    which, cell, values, proofs = cells_under(W, labels)
    cs = commitments_of(W, S)
    assert lib.host_kzg_check_cells_layout(*args_of(W, which, cell, values, proofs, commitments=cs), seed=SEED)["ok"] == 1
    cs[c] = W["commitments"][(c + 1) % 8]
    got = lib.host_kzg_check_cells_layout(*args_of(W, which, cell, values, proofs, commitments=cs), seed=SEED)
    assert got["ok"] == 0 and got["first_failing"] == -1 and got["bad_points"] == 0, got
    got = lib.host_kzg_check_cells_layout(*args_of(W, which, cell, values, proofs, commitments=cs), seed=SEED, locate=True)
    assert got["ok"] == 0 and got["first_failing"] == t and got["rounds"] >= 2, got
    V = rows_world(W, 70)  # the same in the open-cosets form: row 66
    cs = V["commitments"].copy()
    cs[66] = W["commitments"][(66 + 1) % 8]
    got = lib.host_kzg_check_open_cosets_layout(*cosets_args(V, commitments=cs), seed=SEED, locate=True)
    assert got["ok"] == 0 and got["first_failing"] == 66 * W["m"], got
    assert got == lib.host_kzg_check_cells_layout(*args_of(V, *cosets_as_labelled(V), commitments=cs), seed=SEED, locate=True)


def test_argument_errors(lib, oracle, worlds):
    """the bounds on the commitments of all four layout entries; the other verdicts are the shared text's (tests/test_kzg_check_cells_host.py)"""
    from barretenberg_amd import BbGpuError
    from barretenberg_amd.bbgpu import KzgCheckReport, _ptr, u64p
    W = worlds(16, 4)
    n, l, S = 16, 4, 70
    which, cell, values, proofs = cells_under(W, mixed(S, 12))
    cs = commitments_of(W, S)
    u32p = C.POINTER(C.c_uint32)
    rep, seed, keep = KzgCheckReport(), aligned_copy(SEED), []

    def u32(w):
        keep.append(np.ascontiguousarray(w, dtype=np.uint32))
        return keep[-1].ctypes.data_as(u32p)

    def call(fn, good, **changes):
        a = list(good)
        for k, v in changes.items():
            a[int(k[1:])] = v
        return fn(*a)

    for fn in (lib.lib.bbgpu_kzg_check_cells_layout, lib.lib.bbgpu_host_kzg_check_cells_layout):
        fn.argtypes = [u64p, C.c_size_t, u32p, u32p, u64p, u64p, C.c_size_t, C.c_size_t, C.c_size_t, u64p, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        good = [_ptr(cs), S, u32(which), u32(cell), _ptr(values), _ptr(proofs), 12, n, l, _ptr(W["head"]), _ptr(W["g2_xl"]), _ptr(seed), 0, C.byref(rep)]
        for num in (0, MAX_S + 1):
            assert call(fn, good, a1=num) == -3 and b"65536 shared commitments" in lib.lib.bbgpu_last_error(), num
        assert call(fn, good, a1=int(which.max())) == -3 and b"names no commitment" in lib.lib.bbgpu_last_error()  # a label equal to S
        w2 = which.copy()
        w2[5] = S
        assert call(fn, good, a2=u32(w2)) == -3 and b"cell 5" in lib.lib.bbgpu_last_error()
        assert call(fn, good, a0=None) == -3 and call(fn, good, a6=0) == -2 and call(fn, good, a8=3) == -2  # the shared verdicts still hold
        if fn is lib.lib.bbgpu_host_kzg_check_cells_layout:
            assert call(fn, good) == 0 and rep.ok == 1 and rep.count == 12
    V = rows_world(W, 70)
    vals, prf = aligned_copy(V["values"].reshape(-1, 4)), aligned_copy(V["proofs"].reshape(-1, 8))
    for fn in (lib.lib.bbgpu_kzg_check_open_cosets_layout, lib.lib.bbgpu_host_kzg_check_open_cosets_layout):
        fn.argtypes = [u64p, u64p, C.c_size_t, u64p, C.c_size_t, C.c_size_t, C.c_int, u64p, u64p, u64p, C.c_int, C.POINTER(KzgCheckReport)]
        good = [_ptr(V["commitments"]), _ptr(vals), n, _ptr(prf), n, l, 70, _ptr(W["head"]), _ptr(W["g2_xl"]), _ptr(seed), 0, C.byref(rep)]
        for batch in (0, -1, MAX_S + 1):
            assert call(fn, good, a6=batch) == -2 and b"batch <= 65536" in lib.lib.bbgpu_last_error(), batch
        assert call(fn, good, a6=MAX_S, a4=32, a2=32) == -2  # batch x n = 2^21
        assert call(fn, good, a4=1 << 15, a2=1 << 15, a6=33) == -2 and call(fn, good, a2=n - 1) == -2
        assert call(fn, good, a0=None) == -3
        if fn is lib.lib.bbgpu_host_kzg_check_open_cosets_layout:
            assert call(fn, good) == 0 and rep.ok == 1 and rep.count == 70 * W["m"]
    # the entries of 64 commitments refuse what they refused
    a = args_of(W, which, cell, values, proofs, commitments=cs)
    for fn in (lib.kzg_check_cells, lib.host_kzg_check_cells):
        with pytest.raises(BbGpuError, match=cases.ERR_ARG + " KZG check: 1 .. 64 shared commitments"):
            fn(*a, seed=SEED)
    for fn in (lib.kzg_check_open_cosets, lib.host_kzg_check_open_cosets):
        with pytest.raises(BbGpuError, match=cases.ERR_SIZE + " KZG check"):
            fn(*cosets_args(V), seed=SEED)
    with pytest.raises(ValueError):
        lib.host_kzg_check_open_cosets_layout(*cosets_args(V), batch=71, seed=SEED)  # the binding checks its arrays up to the new cap
