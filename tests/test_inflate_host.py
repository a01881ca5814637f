"""The DEFLATE core (basecount_amd/csrc/bc_inflate.h) compiled for the host with AddressSanitizer and
UBSan, as a stand-alone program (tests/native/inflate_check.cpp): every vector of
tests/inflate_vectors.py, 64 guard bytes around input and output, against zlib."""
import os
import subprocess
import tempfile

import pytest

import inflate_vectors as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results():
    src = os.path.join(REPO, "tests", "native", "inflate_check.cpp")
    vecs = V.VALID + V.INVALID
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "inflate_check")
        try:
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("inflate_check.cpp does not compile:\n" + e.stderr)
        vin, vout = os.path.join(tmp, "vectors.bin"), os.path.join(tmp, "results.bin")
        with open(vin, "wb") as f:
            f.write(V.pack_file(vecs))
        r = subprocess.run([exe, vin, vout], capture_output=True, text=True, timeout=120)
        # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        assert r.stdout.startswith("ok %d vectors" % len(vecs))
        with open(vout, "rb") as f:
            res = V.unpack_results(f.read(), vecs)
    return dict(zip((x.name for x in vecs), res))


def test_vector_names_are_unique():
    names = [x.name for x in V.VALID + V.INVALID]
    assert len(set(names)) == len(names)


def test_valid_streams_inflate_to_zlibs_bytes(results):
    for x in V.VALID:
        status, guards, out = results[x.name]
        assert guards == 1, x.name
        assert status == 0, "%s: status %d" % (x.name, status)
        assert out == x.expect, x.name


def test_invalid_streams_never_accepted_unless_zlib_accepts(results):
    """Both directions (V.check_rule): refused where zlib refuses, zlib's bytes where it accepts."""
    refused = 0
    for x in V.INVALID:
        status, guards, out = results[x.name]
        assert guards == 1, x.name
        V.check_rule(x, status, out)
        refused += status != 0
    assert refused > len(V.INVALID) // 2  # the list is what it says


def test_named_invalid_streams_are_refused(results):
    for name in V.NAMED_INVALID:
        assert results[name][0] != 0, name
