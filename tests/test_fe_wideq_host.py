"""The wide quotient-digit forms of csrc/fe.hpp (32-bit digits 0..7 of the Montgomery reduction, the top digit masked) against big-integer
arithmetic: tests/cpp/test_fe_wideq.cpp, a stand-alone program with its own main, built with AddressSanitizer + UBSan and run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_quotient_forms_against_big_integers(tmp_path):
    """Fq and Fr, all seven forms, operands at the corners of the declared bounds: exact Montgomery relation, result below the declared bound,
    exact limbs, canonicalisation, and the 64-bit columns beside a 128-bit walk (also with all nine limbs at the form's maximum)"""
    exe = str(tmp_path / "bbgpu_test_fe_wideq")
    src = os.path.join(ROOT, "tests", "cpp", "test_fe_wideq.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ALL OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
