"""The one-op chunk setup of k_pileup's slice instance (bc_slice::covered_one_op in
basecount_amd/csrc/bc_slice.h, decode_one_op in bc_runs.h) compiled for the host with
AddressSanitizer and UBSan, as a stand-alone program (tests/native/one_op_check.cpp): the coverage
predicate over three issued pieces against bc_slice::covered and a restatement from the
definitions, and the one-word decode against decode_runs<1>, enumerated over sequence alignments,
read starts, lengths, buffer ends and all 16 op codes."""
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output():
    src = os.path.join(REPO, "tests", "native", "one_op_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "one_op_check")
        try:
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("one_op_check.cpp does not compile:\n" + e.stderr)
        return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_one_op_setup_runs_clean_under_the_sanitizers(output):
    # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
    assert output.returncode == 0 and output.stderr == "", output.stdout + output.stderr
    words = output.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 10**7, output.stdout


def test_the_header_names_three_pieces():
    """bc_tile.h masks piece 3's lanes by the header's count; the slot's stride stays 64 B."""
    text = open(os.path.join(REPO, "basecount_amd", "csrc", "bc_slice.h")).read()
    assert "kOneOpPieces = 3" in text and "kSlotBytes = 64" in text and "kPieceBytes = 16" in text
    tile = open(os.path.join(REPO, "basecount_amd", "csrc", "bc_tile.h")).read()
    assert "bc_slice::kOneOpPieces" in tile and "bc_slice::covered_one_op" in tile and "decode_one_op" in tile
