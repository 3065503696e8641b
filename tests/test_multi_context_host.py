"""CPU tests of the device contexts of bbgpu_init_devices: the split policy of csrc/multi_plan.hpp compiled on its own, and the argument
checks of bbgpu_init_devices, which hold before any HIP call (and so on a machine without a GPU)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, (1 << 16) - 1, 1 << 16, (1 << 17) - 1, 1 << 17, 3 * (1 << 16) + 5, 1 << 20, (1 << 21) + 3]

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "multi_plan.hpp"
int main(int argc, char** argv)
{
    for (int a = 1; a < argc; a++) {
        const size_t n = strtoull(argv[a], nullptr, 0);
        for (int count = 1; count <= 8; count++) {
            bbgpu::multi::Slice s[8];
            const int m = bbgpu::multi::plan_slices(n, count, s);
            printf("%zu %d %d", n, count, m);
            for (int k = 0; k < m; k++) printf(" %d:%zu:%zu", s[k].context, s[k].first, s[k].len);
            printf("\n");
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def lib():
    from barretenberg_amd import BbGpu, build_library
    build_library()
    return BbGpu(init=False)


def test_split_plan_tiles_every_size(tmp_path):
    src = tmp_path / "plan_driver.cpp"
    src.write_text(DRIVER)
    exe = str(tmp_path / "plan_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "barretenberg_amd", "csrc"), "-o", exe, str(src)], check=True)
    out = subprocess.run([exe] + [str(n) for n in SIZES], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [r.split() for r in out if r]
    assert len(rows) == len(SIZES) * 8
    for r in rows:
        n, count, m = int(r[0]), int(r[1]), int(r[2])
        slices = [tuple(int(v) for v in t.split(":")) for t in r[3:]]
        assert m == min(count, max(1, n >> 16)) == len(slices), r
        assert [s[0] for s in slices] == list(range(m)), r          # context order
        pos = 0
        for _, first, length in slices:                            # [0, n) tiled exactly, in order
            assert first == pos, r
            pos += length
        assert pos == n, r
        if m > 1:
            assert min(s[2] for s in slices) >= 1 << 16, r
        if count == 1:
            assert slices == [(0, 0, n)], r


def test_init_devices_argument_errors(lib):
    L = lib.lib
    L.bbgpu_init_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    one = (C.c_int * 1)(0)
    nine = (C.c_int * 9)(*([0] * 9))
    neg = (C.c_int * 2)(0, -1)
    for devices, count in ((None, 1), (one, 0), (nine, 9), (neg, 2), (one, -1)):
        assert L.bbgpu_init_devices(devices, count) == -3, (devices, count)  # BBGPU_ERR_ARG, before any HIP call
        assert L.bbgpu_last_error().decode().startswith("bbgpu_init_devices:")
    assert L.bbgpu_num_contexts() == 1


def test_init_devices_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = lib.lib
    L.bbgpu_init_devices.argtypes = [C.POINTER(C.c_int), C.c_int]
    assert L.bbgpu_init_devices((C.c_int * 2)(0, 0), 2) == -1  # BBGPU_ERR_HIP
    assert "no HIP device" in L.bbgpu_last_error().decode()
    assert L.bbgpu_num_contexts() == 1
    from barretenberg_amd.bbgpu import BbGpuError
    from barretenberg_amd import BbGpu
    with pytest.raises(BbGpuError, match="no HIP device"):
        BbGpu(devices=[0, 0])
