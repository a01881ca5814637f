"""The read selection (basecount_amd/csrc/bc_select.h) compiled for the host with AddressSanitizer
and UBSan, as a stand-alone program (tests/native/select_check.cpp): the kernels' schedule restated
as loops over the same functions.  Every output must equal select_ref's (tests/select_inputs.py,
pinned to bcio_select by tests/test_select_ref.py), with 64 guard bytes around every input and
output and the outputs poisoned, so an unwritten or an overwritten slot shows."""
import os
import subprocess
import tempfile

import pytest

import select_inputs as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = S.cases()


@pytest.fixture(scope="module")
def results():
    """All cases through one run of the program: {name: outputs}."""
    src = os.path.join(REPO, "tests", "native", "select_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "select_check")
        try:
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("select_check.cpp does not compile:\n" + e.stderr)
        vin, vout = os.path.join(tmp, "input.bin"), os.path.join(tmp, "results.bin")
        with open(vin, "wb") as f:
            f.write(S.pack_input(CASES))
        r = subprocess.run([exe, vin, vout], capture_output=True, text=True, timeout=300)
        # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        assert r.stdout.startswith("ok %d cases" % len(CASES))
        with open(vout, "rb") as f:
            res = S.unpack_results(f.read(), CASES)
    return {c[0]: r for c, r in zip(CASES, res)}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_twin_equals_the_reference_selection(results, case):
    name, a, mmq, ref_sel, ref_len, status = case
    got = results[name]
    exp = S.select_ref(a, mmq, ref_sel, ref_len)
    assert exp["status"] == status, "%s: the case was built for status %d" % (name, status)
    assert got["guards"] == 1, name
    S.assert_matches(got, exp, name)


def test_the_cases_cover_what_they_are_named_for():
    """The generated inputs really hold the edges the kernels can break on."""
    by = {c[0]: S.select_ref(c[1], c[2], c[3], c[4]) for c in CASES}
    assert by["n0"]["n_selected"] == 0 and by["none_accepted"]["n_accepted"] == 0
    assert by["none_wanted"]["n_selected"] == 0 and by["none_wanted"]["keyerror_ordinal"] == 0
    assert by["keyerror_first"]["keyerror_rec"] == 0
    last = by["keyerror_last"]
    assert last["keyerror_rec"] == S.RUN + 69 and last["keyerror_ordinal"] == S.RUN + 69
    assert by["keyerror_after_unmapped"]["keyerror_rec"] == 5 and by["keyerror_after_unmapped"]["keyerror_ordinal"] == 1
    assert int((by["thousand_refs_seven_with_reads"]["n_reads"] > 0).sum()) == 7
    assert by["pos_decrease_at_wave_boundary"]["flags"][0] == S.F_INSIDE
    assert list(by["pos_decrease_across_references"]["flags"]) == [S.F_SORTED | S.F_INSIDE] * 2
    assert list(by["inside_edges"]["flags"]) == [3, S.F_SORTED, 3] and by["inside_edges"]["max_end"][2] == 2**32 - 6
    assert by["negative_pos_and_rec_err"]["batch_err_or"] == 24
    for c in CASES:
        cn = by[c[0]]["cig_n"]
        if c[0].startswith("n") and cn.size > 100:
            assert (cn == 8).any() and (cn == 9).any() and (by[c[0]]["qlen"] == 0).any()
