"""prefix_check (csrc/host_random_check.hpp): the verdict and the prefix bisection shared by bbgpu_srs_check, bbgpu_srs_lagrange_check, the batched PLONK
verifier and the KZG checks, driven on its own with fake sums (tests/cpp/test_prefix_check_host.cpp).  No GPU, no library: the header alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prefix_check_under_sanitizers(tmp_path):
    """Every count in 1..9 and 1000, every first failing item and "nothing fails", with and without LOCATE: the verdict, the item found, the rounds counted
    and bounded by 1 + ceil(log2 count), every round inside [1, count] and the first over the whole input, the first round's sums kept; an error from any of
    the four rounds of (count 8, item 2) ends the check at once.  Built with AddressSanitizer + UBSan (CPU build, its own main, no preloaded runtime)."""
    exe = str(tmp_path / "bbgpu_test_prefix_check_host")
    base = ["g++", "-std=c++17", "-O1", "-g"]
    tail = ["-o", exe, os.path.join(ROOT, "tests", "cpp", "test_prefix_check_host.cpp")]
    b = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + tail, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr or "ubsan" in b.stderr or "sanitize" in b.stderr):
        b = subprocess.run(base + tail, capture_output=True, text=True)  # an image without the sanitizer runtime still runs the program
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
