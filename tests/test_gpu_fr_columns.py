"""bbgpu_fr_ntt_columns_device and bbgpu_fr_recover_columns_device on the GPU (-m gpu): k_fr_cols_tables and k_fr_cols_decode of csrc/fr_columns.hip,
k_g1_roots and k_g1_vanish_cols through the new driver, and the drivers in capi.hip against the host twins bit for bit -- the whole matrix with its padding,
the report and first_bad.  The twins are held to the definition by tests/test_fr_columns_host.py.  Shapes sit where the tile arithmetic can go wrong, not
at workload size: a tile is C = 2048 / rows columns, and every C from 1024 to 1 runs at widths 1, C - 1, C, C + 1 and 2 C + 3 with a padded stride; sets
that are no power of two and straddle tile edges; missing counts around the 256-root tile of k_g1_vanish_cols; the degree bounds at their ends; altered
elements at tile edges; non-canonical inputs; one larger shape; a round trip with the group side; a non-default stream; and the error contract under
injected failures of the four host-side funnels (no failure is provoked on the device), with what a failed call may have written."""
import numpy as np
import pytest

from tests.fr_columns_cases import (JUNK, NONE, PAD, SENTINEL, add_modulus_where_it_fits, alter, clean_report, codeword_ints, codeword_memory, erase,
                                    matrix_memory, missing_mask, random_elements, row_sets)

pytestmark = pytest.mark.gpu
KINDS = ("alloc", "h2d", "d2h", "launch")
KEYS = {"alloc": "alloc_calls", "h2d": "h2d_calls", "d2h": "d2h_calls", "launch": "launch_checks"}
FAR = 1 << 62
# the funnels one warm bbgpu_fr_recover_columns_device with first_bad_out passes (include/bbgpu.h): allocations -- the lists; z, z', the tables and the
# roots; the call's two findings; the per-column findings; uploads -- the lists, the findings' start; read-backs -- the two findings, the per-column
# findings; launch checks -- k_g1_roots with k_g1_vanish_cols, the batch inversion's two scans and its product, k_fr_cols_tables, k_fr_cols_decode
WARM = dict(alloc_calls=4, h2d_calls=2, d2h_calls=2, launch_checks=6)
WARM_NTT = dict(alloc_calls=1, h2d_calls=0, d2h_calls=0, launch_checks=2)  # the twiddles; k_fr_cols_tables, k_fr_cols_decode<false>
DECODE_LAUNCH = 5  # the index of the decode's launch check among the six


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    yield g
    g.fault_inject(None)
    g.shutdown()


def resident(mem):
    import torch
    return torch.from_numpy(mem.view(np.int64)).cuda()


def host_of(t):
    return t.cpu().numpy().view(np.uint64)


def both(lib, sets_rows, held, rows, width, stride, d, stream=None):
    """the device entry on a resident copy against the twin on a host copy: the whole matrix, the report, first_bad"""
    dev = resident(held)
    rep, first_bad = lib.fr_recover_columns_device(sets_rows, dev.data_ptr(), rows, width, d, stride=stride, stream=stream)
    want = held.copy()
    want_rep, want_bad = lib.host_fr_recover_columns(sets_rows, want, rows, width, d, stride=stride)
    got = host_of(dev)
    assert np.array_equal(got, want) and rep == want_rep and np.array_equal(first_bad, want_bad), (rep, want_rep)
    return got, rep, first_bad


def tile_widths(rows):
    C = 2048 // rows
    return sorted({max(1, w) for w in (1, C - 1, C, C + 1, 2 * C + 3)})


TILES = [(rows, width) for rows in (2, 4, 8, 64, 512, 1024, 2048) for width in tile_widths(rows)]


@pytest.mark.parametrize("rows,width", TILES, ids=["%dx%d" % t for t in TILES])
def test_every_tile_shape_both_entries_both_kinds(lib, rows, width):
    stride, d = width + PAD, max(1, rows // 2)
    full = codeword_memory(lib, rows, width, d, stride, seed=width)
    sets = min(3, width)
    mus = [(rows - d, 0, max(1, (rows - d) // 3))[s] for s in range(sets)]
    sets_rows = row_sets(rows, mus)
    got, rep, first_bad = both(lib, sets_rows, erase(full, rows, width, stride, sets_rows), rows, width, stride, d)
    assert np.array_equal(got, full) and rep == clean_report(rows, sets_rows) and np.all(first_bad == NONE)
    for kind in ("fft", "ifft"):
        mem = full.copy()
        mem.reshape(rows, stride, 4)[:, :width] = random_elements(rows * width, rows + width).reshape(rows, width, 4)
        dev = resident(mem)
        lib.fr_ntt_columns_device(dev.data_ptr(), rows, width, kind, stride=stride)
        assert np.array_equal(host_of(dev), lib.host_fr_ntt_columns(mem, rows, width, kind, stride=stride)), kind
        assert np.all(mem.reshape(rows, stride, 4)[:, width:] == np.uint64(SENTINEL))


@pytest.mark.parametrize("rows,width", [(8, 259), (512, 67)])
@pytest.mark.parametrize("sets", [1, 2, 3, 64, "width"])
def test_sets_that_straddle_tiles_with_different_missing_counts(lib, rows, width, sets):
    sets = width if sets == "width" else sets
    stride, d = width + PAD, rows // 4
    full = codeword_memory(lib, rows, width, d, stride, seed=sets)
    cycle = (rows - d, 0, 1, rows // 2, rows - d - 1)  # one set at mu_s = rows - d, one that misses nothing
    sets_rows = row_sets(rows, [cycle[s % len(cycle)] for s in range(sets)])
    got, rep, first_bad = both(lib, sets_rows, erase(full, rows, width, stride, sets_rows), rows, width, stride, d)
    assert np.array_equal(got, full) and rep == clean_report(rows, sets_rows) and np.all(first_bad == NONE)


def test_missing_counts_around_the_root_tile_of_the_vanishing_kernel(lib):
    rows, width, d = 1024, 8, 500
    mus = (0, 1, 255, 256, 257, 513)
    stride = width + PAD
    full = codeword_memory(lib, rows, width, d, stride, seed=1)
    sets_rows = row_sets(rows, mus)
    got, rep, first_bad = both(lib, sets_rows, erase(full, rows, width, stride, sets_rows), rows, width, stride, d)
    assert np.array_equal(got, full) and rep == clean_report(rows, sets_rows) and rep["max_missing"] == 513


@pytest.mark.parametrize("rows,d,mus", [(64, 1, (63, 0, 30)), (64, 34, (30, 30)), (64, 64, (0,)), (8, 8, (0, 0))],
                         ids=["d=1", "d=count", "d=rows", "d=rows-8"])
def test_degree_bounds_at_their_ends(lib, rows, d, mus):
    width = 2 * (2048 // rows) + 3
    stride = width + PAD
    full = codeword_memory(lib, rows, width, d, stride, seed=d)
    sets_rows = row_sets(rows, mus)
    held = erase(full, rows, width, stride, sets_rows)
    if d == 34:  # count_s == d: no redundancy, an altered element cannot be seen and is not a finding
        alter(held, stride, int(sets_rows[1][0]), 1)
    got, rep, first_bad = both(lib, sets_rows, held, rows, width, stride, d)
    assert rep == clean_report(rows, sets_rows) and np.all(first_bad == NONE)
    if d != 34:
        assert np.array_equal(got, full)


def test_altered_elements_at_tile_edges_are_found_and_present_rows_stay(lib):
    rows, d = 64, 17
    C = 2048 // rows
    width = 2 * C + 3
    stride = width + PAD
    full = codeword_memory(lib, rows, width, d, stride, seed=9)
    sets_rows = row_sets(rows, (30, 0, 41))
    clean = erase(full, rows, width, stride, sets_rows)
    keep = np.ones((rows, stride), dtype=bool)
    keep[:, :width] = ~missing_mask(rows, width, sets_rows)
    for columns in ((C,), (width - 1,), (C + 1, 5)):  # the first column of a tile; the last column of the matrix; two columns at once
        held = clean.copy()
        for j in columns:
            alter(held, stride, int(sets_rows[j % 3][2]), j)
        got, rep, first_bad = both(lib, sets_rows, held, rows, width, stride, d)  # BBGPU_OK: a finding, not an error
        assert [j for j in range(width) if int(first_bad[j]) != NONE] == sorted(columns)
        assert rep["consistent"] == 0 and rep["first_bad_column"] == min(columns) and rep["first_bad_coeff"] == int(first_bad[min(columns)])
        assert np.array_equal(got.reshape(rows, stride, 4)[keep], held.reshape(rows, stride, 4)[keep])


def test_non_canonical_inputs_give_the_same_outputs(lib):
    rows, d, width = 64, 20, 70
    stride = width + PAD
    full = codeword_memory(lib, rows, width, d, stride, seed=4)
    sets_rows = row_sets(rows, (44, 3, 0, 17))
    held = erase(full, rows, width, stride, sets_rows)
    other, changed = add_modulus_where_it_fits(held)
    assert changed > rows * width // 4
    got, rep, _ = both(lib, sets_rows, other, rows, width, stride, d)
    gone = np.zeros((rows, stride), dtype=bool)
    gone[:, :width] = missing_mask(rows, width, sets_rows)
    g, f, o = got.reshape(rows, stride, 4), full.reshape(rows, stride, 4), other.reshape(rows, stride, 4)
    assert rep == clean_report(rows, sets_rows) and np.array_equal(g[gone], f[gone]) and np.array_equal(g[~gone], o[~gone])


def test_one_larger_shape(lib):
    rows, width, sets, d = 512, 4096, 64, 256
    full = codeword_memory(lib, rows, width, d, width, seed=2)
    sets_rows = row_sets(rows, [256] * sets)
    assert len({tuple(sorted(int(k) for k in r)) for r in sets_rows}) == sets
    got, rep, first_bad = both(lib, sets_rows, erase(full, rows, width, width, sets_rows), rows, width, width, d)
    assert np.array_equal(got, full) and rep == clean_report(rows, sets_rows) and np.all(first_bad == NONE)


def test_round_trip_with_the_group_side(lib):
    """(rows, width) = (8, 64), d = 4, the rows are COEFFICIENT rows: the commitments of the rows recovered here equal the commitments recovered by
    bbgpu_g1_recover from the commitments of the rows one holds, bit for bit"""
    import torch
    from barretenberg_amd.plonk import to_montgomery_limbs
    rows, width, d = 8, 64, 4
    full = matrix_memory(codeword_ints(rows, width, d, seed=5), width)
    handle = lib.srs_generate(to_montgomery_limbs([0x0123456789ABCDEF0F1E2D3C4B5A6978])[0], width)

    def commit(mem):
        dev = resident(mem)
        out = np.stack([lib.msm_device(handle, dev.data_ptr() + 32 * width * r, width)[:8] for r in range(rows)])
        torch.cuda.synchronize()
        return out
    before = commit(full)
    sets_rows = row_sets(rows, (4,))
    dev = resident(erase(full, rows, width, width, sets_rows))
    rep, _ = lib.fr_recover_columns_device(sets_rows, dev.data_ptr(), rows, width, d, want_first_bad=False)
    assert rep == clean_report(rows, sets_rows) and np.array_equal(host_of(dev), full)
    points, grep = lib.g1_recover(sets_rows[0], np.ascontiguousarray(before[sets_rows[0].astype(np.int64)]), rows, d)
    after = commit(host_of(dev))
    assert grep["consistent"] == 1 and np.array_equal(points[0], before) and np.array_equal(after, before)
    lib.srs_release(handle)


def test_a_non_default_stream_gives_the_same_result(lib):
    import torch
    rows, d, width = 64, 17, 67
    stride = width + PAD
    full = codeword_memory(lib, rows, width, d, stride, seed=6)
    sets_rows = row_sets(rows, (30, 0, 41))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    got, rep, _ = both(lib, sets_rows, erase(full, rows, width, stride, sets_rows), rows, width, stride, d, stream=st.cuda_stream)
    assert np.array_equal(got, full) and rep == clean_report(rows, sets_rows)
    dev = resident(full)
    torch.cuda.synchronize()
    lib.fr_ntt_columns_device(dev.data_ptr(), rows, width, "ifft", stride=stride, stream=st.cuda_stream)
    assert np.array_equal(host_of(dev), lib.host_fr_ntt_columns(full.copy(), rows, width, "ifft", stride=stride))


# ---- the error contract under injected failures of the host-side funnels ---------------------------------------------------------------------------------
def warm_case(lib):
    rows, d, width = 8, 4, 300
    stride = width + PAD
    full = codeword_memory(lib, rows, width, d, stride, seed=8)
    sets_rows = row_sets(rows, (4, 3, 1))
    return rows, d, width, stride, sets_rows, full, erase(full, rows, width, stride, sets_rows)


def counted(lib, run, keys):
    lib.fault_inject("launch:%d" % FAR)
    got = run()
    st = lib.fault_stats()
    lib.fault_inject(None)
    return got, {k: st[k] for k in keys}


def test_funnel_counts_of_a_warm_call(lib):
    import torch
    rows, d, width, stride, sets_rows, full, held = warm_case(lib)

    def run(want_first_bad=True):
        dev = resident(held)
        rep, _ = lib.fr_recover_columns_device(sets_rows, dev.data_ptr(), rows, width, d, stride=stride, want_first_bad=want_first_bad)
        torch.cuda.synchronize()
        return rep["consistent"] == 1 and np.array_equal(host_of(dev), full)
    assert run()
    ok, st = counted(lib, run, WARM)
    print("funnels of one warm fr_recover_columns_device at (8, 300, 3), missing 4, 3, 1:", st)
    assert ok and st == WARM
    ok, st = counted(lib, lambda: run(False), WARM)
    assert ok and st == dict(WARM, alloc_calls=3, d2h_calls=1)

    def ntt():
        dev = resident(full)
        lib.fr_ntt_columns_device(dev.data_ptr(), rows, width, "fft", stride=stride)
        return True
    ntt()
    _, st = counted(lib, ntt, WARM_NTT)
    print("funnels of one warm fr_ntt_columns_device:", st)
    assert st == WARM_NTT


@pytest.mark.parametrize("kind", KINDS)
def test_injected_failures_leave_nothing_behind_and_write_only_missing_rows(lib, kind):
    """every site of the funnel `kind` that one warm call passes, failed once.  These are host-side funnels (the library's failure injection of API
    results); nothing faults on the device.  Each failure returns BBGPU_ERR_HIP, leaves no allocation live and report and first_bad as they were, and the
    next call is bit-exact.  What it may have written is what include/bbgpu.h says: nothing where it failed before the decode was launched; missing rows,
    all or part, after that; present rows and padding never."""
    import torch
    from barretenberg_amd import BbGpuError
    rows, d, width, stride, sets_rows, full, held = warm_case(lib)
    keep = np.ones((rows, stride), dtype=bool)
    keep[:, :width] = ~missing_mask(rows, width, sets_rows)

    def run(dev=None):
        dev = resident(held) if dev is None else dev
        rep, first_bad = lib.fr_recover_columns_device(sets_rows, dev.data_ptr(), rows, width, d, stride=stride)
        torch.cuda.synchronize()
        return rep["consistent"] == 1 and np.all(first_bad == NONE) and np.array_equal(host_of(dev), full)
    assert run()  # warm
    _, sites = counted(lib, run, WARM)
    assert sites == WARM
    before = lib.fault_stats()
    for k in range(sites[KEYS[kind]] + 1):  # k == sites: the armed failure no longer fires
        lib.fault_inject("%s:%d" % (kind, k))
        if k < sites[KEYS[kind]]:
            dev = resident(held)
            with pytest.raises(BbGpuError, match=" -1:"):
                run(dev)
            st = lib.fault_stats()
            assert st["fired"] == 1 and st["armed"] == 0 and st["absorbed"] == 0, (kind, k, st)
            torch.cuda.synchronize()
            got = host_of(dev)
            assert np.array_equal(got.reshape(rows, stride, 4)[keep], held.reshape(rows, stride, 4)[keep]), (kind, k)
            launched = kind == "d2h" or (kind == "launch" and k >= DECODE_LAUNCH)
            if not launched:
                assert np.array_equal(got, held), (kind, k)
            else:  # a missing element is as it was or recovered, nothing else
                g, h, f = got.reshape(-1, 4), held.reshape(-1, 4), full.reshape(-1, 4)
                assert np.all(np.all(g == h, axis=1) | np.all(g == f, axis=1)), (kind, k)
        else:
            assert run(), (kind, k)
            st = lib.fault_stats()
            assert st["fired"] == 0 and st["armed"] == 1, (kind, k, st)
        lib.fault_inject(None)
        torch.cuda.synchronize()
        st = lib.fault_stats()
        assert st["slots_pending"] == 0 and st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        assert run(), (kind, k)


def test_injected_failures_of_the_transform_entry(lib):
    import torch
    from barretenberg_amd import BbGpuError
    rows, d, width, stride, sets_rows, full, held = warm_case(lib)
    want = lib.host_fr_ntt_columns(full.copy(), rows, width, "fft", stride=stride)
    before = lib.fault_stats()
    for kind, k in (("alloc", 0), ("launch", 0), ("launch", 1)):
        lib.fault_inject("%s:%d" % (kind, k))
        dev = resident(full)
        with pytest.raises(BbGpuError, match=" -1:"):
            lib.fr_ntt_columns_device(dev.data_ptr(), rows, width, "fft", stride=stride)
        lib.fault_inject(None)
        torch.cuda.synchronize()
        st = lib.fault_stats()
        assert st["live_allocations"] == before["live_allocations"] and st["live_bytes"] == before["live_bytes"], (kind, k, st)
        dev = resident(full)
        lib.fr_ntt_columns_device(dev.data_ptr(), rows, width, "fft", stride=stride)
        assert np.array_equal(host_of(dev), want), (kind, k)


def test_kernel_times_are_reported(lib):
    rows, d, width, stride, sets_rows, full, held = warm_case(lib)
    dev = resident(held)
    lib.set_timing(1)
    try:
        lib.fr_recover_columns_device(sets_rows, dev.data_ptr(), rows, width, d, stride=stride)
        times = lib.last_timing()
    finally:
        lib.set_timing(0)
    assert len(times) == 2 and all(0 < v < 1000 for v in times), times  # the vanishing values with the tables; the decode kernel
