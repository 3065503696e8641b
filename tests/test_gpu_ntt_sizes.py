"""Every transform size the library accepts, 2^1 .. 2^28 (NTT_MAX_LOG2N, the field's two-adicity), all seven kinds, across the input range
the contract promises ("inputs anywhere in [0, 2^256)", ntt.hip): each size-dependent switch of build_domain / launch_pass -- single pass and
the unfused kernel below 16 points, the odd two-pass splits, half tiles below 2^20, the XCD remap from 2^20, LDS twiddles, the three-pass
splits l1 = 8 .. 10 with row domains 2^14 .. 2^18 -- is run against a reference at exactly that size.

  2^1 .. 2^22   vs oracle.ntt on the canonical residues; the device gets three input classes with the same residues: canonical, [0, 2r)
                (tests.util.noncanonical) and max lift (every element at its largest representative below 2^256, raw 0 / r - 1 / r / 2r /
                5r / 2^256 - 1 at fixed positions); all three must give the same, bit-exact output
  2^23, 2^24    the max lift of tests/golden/big_r4.json's input vs its digests (the [0, 2r) input is tests/test_gpu_parity.py's)
  2^25 .. 2^28  vs tests/golden/ntt_large.json (tools/gen_golden_ntt_large.py, the reference itself): max lift at every size, [0, 2r) at
                2^25 and 2^26
  batched       bbgpu_ntt_device_batch at 2^16, 2^20 (two-pass batched launch, without / with XCD remap) and 2^23 (the three-pass loop)

One 2^28 vector is 8 GiB of host memory: the large sizes keep one pristine input and one working copy, hash in place and drop both
before the next size."""
import numpy as np
import pytest

from oracle.pyoracle import FR_MODULUS, NTT_KINDS, from_int
from tests.util import (CONST_SEED, NTT_SEED, extreme_positions, lift_extremes, lift_max, limbs, noncanonical, sha_inplace)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from barretenberg_amd import BbGpu
    g = BbGpu(device=0)
    g.set_host_thresholds(0, 0)  # every size on the device kernels
    yield g
    g.shutdown()


@pytest.fixture(scope="module")
def const(oracle):
    return oracle.random_scalars(CONST_SEED, 1)[0]


def first_mismatch(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return int(bad[0]) if bad.size else None


def check_equal(got, want, what):
    i = first_mismatch(got, want)
    assert i is None, "%s: first mismatch at index %d of %d (%d elements differ)" % (what, i, want.shape[0],
                                                                                  int((got != want).any(axis=1).sum()))


def input_classes(residues):
    """(name, input) pairs with the residues of the canonical `residues`"""
    n = residues.shape[0]
    lifted = lift_max(residues.copy(), FR_MODULUS)
    for i, v in zip(extreme_positions(n, 6), lift_extremes(FR_MODULUS)):
        lifted[i] = from_int(v)
    return [("canonical", residues), ("[0, 2r)", noncanonical(residues, FR_MODULUS)), ("max lift", lifted)]


def canonical_residues(oracle, seed, n):
    """seeded canonical elements; the positions of the raw extremes hold the extremes' residues"""
    co = oracle.random_scalars(seed, n)
    for i, v in zip(extreme_positions(n, 6), lift_extremes(FR_MODULUS)):
        co[i] = from_int(v % FR_MODULUS)
    return co


# ------------------------------------------------------------------ one and two passes: vs the oracle ---------------------------
@pytest.mark.parametrize("log2n", range(1, 23))
def test_ntt_every_size_all_kinds_all_input_classes(gpu, oracle, const, log2n):
    n = 1 << log2n
    co = canonical_residues(oracle, NTT_SEED + 1000 + log2n, n)
    classes = input_classes(co)
    for kind in NTT_KINDS:
        want = oracle.ntt(co, kind, const)
        for cls, x in classes:
            got = gpu.ntt(x.copy(), kind, const)
            check_equal(got, want, "2^%d %s, %s input" % (log2n, kind, cls))


# ------------------------------------------------------------------ three passes: vs the reference's digests --------------------
def check_digests(gpu, pristine, work, cases, c, log2n, cls):
    """every case (one kind) on a copy of `pristine` in `work`, hashed in place"""
    for case in cases:
        np.copyto(work, pristine)
        gpu.ntt(work, case["kind"], c)
        for i, v in case["samples"].items():
            assert np.array_equal(work[int(i)], limbs(v)), "2^%d %s, %s input: sample %s" % (log2n, case["kind"], cls, i)
        assert sha_inplace(work) == case["sha256"], "2^%d %s, %s input: sha256" % (log2n, case["kind"], cls)


@pytest.mark.parametrize("log2n", [23, 24])
def test_ntt_max_lift_extended_domain_sizes(gpu, oracle, golden, log2n):
    """the max lift of big_r4.json's input (noncanonical_fast: same residues) must give the reference's outputs, all seven kinds"""
    g = golden("big_r4.json")
    n = 1 << log2n
    cases = [x for x in g["ntt"] if x["n"] == n]
    assert len(cases) == len(NTT_KINDS)
    pristine = lift_max(noncanonical(oracle.random_scalars(NTT_SEED, n), FR_MODULUS), FR_MODULUS)
    work = np.empty_like(pristine)
    check_digests(gpu, pristine, work, cases, limbs(g["constant"]), log2n, "max lift")


@pytest.mark.parametrize("log2n", [25, 26, 27, 28])
def test_ntt_largest_sizes_vs_reference(gpu, oracle, golden, log2n):
    """2^25 .. 2^28: pass A of 2^9 / 2^10 points, row domains of 2^16 / 2^18 -- the reference's digests (tests/golden/ntt_large.json)"""
    g = golden("ntt_large.json")
    n = 1 << log2n
    cases = [x for x in g["ntt"] if x["n"] == n]
    assert len(cases) == len(NTT_KINDS)
    assert limbs(g["constant"]).tolist() == oracle.random_scalars(int(g["constant_seed"], 16), 1)[0].tolist()
    pristine = noncanonical(oracle.random_scalars(int(g["ntt_seed"], 16), n), FR_MODULUS)  # the input the reference was given
    work = np.empty_like(pristine)
    if log2n <= 26:
        check_digests(gpu, pristine, work, cases, limbs(g["constant"]), log2n, "[0, 2r)")
    lift_max(pristine, FR_MODULUS)
    check_digests(gpu, pristine, work, cases, limbs(g["constant"]), log2n, "max lift")
    del pristine, work


# ------------------------------------------------------------------ batched entry -----------------------------------------------
@pytest.mark.parametrize("log2n", [16, 20, 23])
def test_ntt_batched_launch_large_sizes(gpu, oracle, const, log2n):
    """bbgpu_ntt_device_batch, batch 3, padded stride, max-lift inputs (the gaps too): every slice equals the oracle (2^16, 2^20) or
    the single transform (2^23, whose single transform the fixtures pin), the gaps stay untouched"""
    import torch
    n, batch, stride = 1 << log2n, 3, (1 << log2n) + 24
    co = oracle.random_scalars(NTT_SEED + 177 + log2n, batch * stride)
    x = lift_max(co.copy(), FR_MODULUS)
    for kind in NTT_KINDS:
        d = torch.from_numpy(x.view(np.int64)).cuda()
        gpu.ntt_device_batch(d.data_ptr(), n, batch, kind, const, stride=stride)
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(np.uint64)
        del d
        for j in range(batch):
            sl = slice(j * stride, j * stride + n)
            want = oracle.ntt(co[sl], kind, const) if log2n <= 22 else gpu.ntt(x[sl].copy(), kind, const)
            check_equal(got[sl], want, "2^%d %s, batch item %d" % (log2n, kind, j))
            assert np.array_equal(got[j * stride + n:(j + 1) * stride], x[j * stride + n:(j + 1) * stride]), (log2n, kind, j)
