"""The tiled walk's bit-plane counters (basecount_amd/csrc/bc_planes.h: planes_add2, planes_join,
planes_counts, fix_n / fix_d) compiled for the host from the same header and checked against a
scalar count over random sequences of all 16 nibble values and of the seven event classes, at
every depth up to the counters' capacities (tests/native/planes_check.cpp)."""
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_counters_match_scalar_counts():
    src = os.path.join(REPO, "tests", "native", "planes_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "planes_check")
        try:
            subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
