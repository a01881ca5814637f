"""The decisions a cohort run shares between its kernels and the host (basecount_amd/csrc/
bc_cohort.h) compiled for the host with AddressSanitizer and UBSan, as a stand-alone program
(tests/native/cohort_check.cpp): the window clip and emptiness (lo < 0, hi >= L, lo > hi, a window
wholly past L), k1 / k2 (n = 1, 2, 511, 512, 513, ...), the segment lookup across empty segments,
and the rebase kernel's schedule as plain loops with sums up to 2^32 - 1 and the refusal at 2^32.
The same constants are pinned on the Python side, where the planner restates them."""
import os
import subprocess
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def output():
    src = os.path.join(REPO, "tests", "native", "cohort_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "cohort_check")
        try:
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("cohort_check.cpp does not compile:\n" + e.stderr)
        return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_host_twin_runs_clean_under_the_sanitizers(output):
    # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
    assert output.returncode == 0 and output.stderr == "", output.stdout + output.stderr
    assert output.stdout.startswith("ok ") and int(output.stdout.split()[1]) > 1000


def test_the_planner_restates_the_headers_limits():
    """plan_cohort cuts where bcc_fits refuses: the header's 2^32 and the Python constant agree, and
    so does the sorted windows' size with the kernel's."""
    from basecount_amd import cohort

    with open(os.path.join(REPO, "basecount_amd", "csrc", "bc_cohort.h")) as fh:
        src = fh.read()
    assert "#define BCC_INDEX_LIMIT 0x100000000ull" in src and cohort.INDEX_LIMIT == 1 << 32
    assert "#define BCC_SORT_MAX 512" in src
    assert cohort.READS_LIMIT == 1 << 31
