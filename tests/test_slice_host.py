"""The slot arithmetic of k_pileup's slice instance (basecount_amd/csrc/bc_slice.h) compiled for the
host with AddressSanitizer and UBSan, as a stand-alone program (tests/native/slice_check.cpp): the
slot's source byte, the record's bit index and the coverage predicate enumerated over read starts,
sequence alignments, run starts, query offsets, run lengths and buffer ends, against a restatement
from the definitions."""
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output():
    src = os.path.join(REPO, "tests", "native", "slice_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "slice_check")
        try:
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("slice_check.cpp does not compile:\n" + e.stderr)
        return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_slot_arithmetic_runs_clean_under_the_sanitizers(output):
    # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
    assert output.returncode == 0 and output.stderr == "", output.stdout + output.stderr
    words = output.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 10**9, output.stdout


def test_the_header_and_the_kernels_agree_on_the_stage():
    """bc_tile.h takes the stage's size from the header; the binding's LDS formula restates it."""
    from basecount_amd import device as D
    text = open(os.path.join(REPO, "basecount_amd", "csrc", "bc_slice.h")).read()
    assert "kSlotBytes = 64" in text and "kSlots = 64" in text and "kPieceBytes = 16" in text
    assert D.slice_lds_bytes(4, 4) == 4 * (1024 + 64 * 64 + 32) + 1536 + 2048 + 64 == 24_256
