#!/usr/bin/env python3
"""tests/golden/reference_build.json: what two host tests of tests/test_host_boundary.py compare against, taken from the reference build
(oracle/_ref, compiled by oracle/Makefile) so that the tests also run where that build is absent:
  * externs: the defined text symbols of polynomial_arithmetic.o and scalar_multiplication.o (the two translation units the shim replaces);
  * transcript: the reference-written oracle/_ref/transcript.dat (plonk_cpu transcript, secret of oracle/plonk_driver.cpp) -- its manifest
    bytes, the SHA-256 of its first 1024 G1 points and its two G2 points.
The tests compare this file with the live build whenever oracle/_ref is present."""
import hashlib
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
OBJECTS = {"polynomial_arithmetic": os.path.join("polynomials", "polynomial_arithmetic.o"),
           "scalar_multiplication": os.path.join("curves", "bn254", "scalar_multiplication.o")}
G1_POINTS = 1024


def externs(path, dynamic=False):
    """defined text symbols of the barretenberg namespace in an object / shared library"""
    out = subprocess.run(["nm"] + (["-D"] if dynamic else []) + ["--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and "barretenberg" in l.split()[2]}


def transcript_facts(data):
    """manifest (28 bytes: seven big-endian u32), SHA-256 of the first G1_POINTS G1 points, the two G2 points after all G1 points"""
    num = int.from_bytes(data[16:20], "big")
    return {"manifest_hex": data[0:28].hex(), "g1_prefix_points": G1_POINTS, "g1_prefix_sha256": hashlib.sha256(data[28:28 + 64 * G1_POINTS]).hexdigest(),
            "g2_hex": data[28 + 64 * num:][:256].hex()}


def main():
    out = {"generator": "tools/gen_ref_build_golden.py (reference build oracle/_ref)",
           "externs": {k: sorted(externs(os.path.join(REF, "obj", p))) for k, p in OBJECTS.items()},
           "transcript": transcript_facts(open(os.path.join(REF, "transcript.dat"), "rb").read())}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "reference_build.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
