"""The row formatter (basecount_amd/csrc/bc_fmt.h) compiled for the host with AddressSanitizer and
UBSan, as a stand-alone program (tests/native/fmt_check.cpp): the kernels' schedule restated as
loops over the same functions.  Every case's text, seg_off, total and status must equal rows_ref's
(tests/fmt_inputs.py: fmt.rows_text per segment), with 64 guard bytes around every buffer and the
outputs poisoned; a scalar sweep compares the rounding with bcio_fmt_pyround_float."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fmt_inputs as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = F.cases()
REFS = {}


def ref_of(c):
    if c["name"] not in REFS:
        REFS[c["name"]] = F.rows_ref(c)
    return REFS[c["name"]]


def cap_of(c):
    """The text buffer of a case: exactly the text, so a byte written past the total lands in the guard."""
    return len(ref_of(c)[0])


@pytest.fixture(scope="module")
def exe():
    src = os.path.join(REPO, "tests", "native", "fmt_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fmt_check")
        try:
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", path, "-ldl"],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("fmt_check.cpp does not compile:\n" + e.stderr)
        yield path


def run_cases(exe, cs, caps):
    with tempfile.TemporaryDirectory() as tmp:
        vin, vout = os.path.join(tmp, "input.bin"), os.path.join(tmp, "results.bin")
        with open(vin, "wb") as f:
            f.write(F.pack_input(cs, caps))
        r = subprocess.run([exe, "cases", vin, vout], capture_output=True, text=True, timeout=300)
        # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
        assert r.stdout.startswith("ok %d cases" % len(cs))
        with open(vout, "rb") as f:
            return F.unpack_results(f.read(), cs, caps)


@pytest.fixture(scope="module")
def results(exe):
    """All cases through one run of the program, each with a text buffer of exactly its text."""
    return {c["name"]: r for c, r in zip(CASES, run_cases(exe, CASES, [cap_of(c) for c in CASES]))}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_equals_the_host_formatter(results, case):
    got = results[case["name"]]
    text, seg_off = ref_of(case)
    assert got["guards"] == 1
    assert got["status"] == case["status"] and got["declined"] == case["declined"]
    if case["status"] == F.ST_OK:
        assert got["total"] == len(text)
        assert np.array_equal(got["seg_off"], seg_off)
        assert got["text"] == text
    else:  # declined (the total of a text with a declined value means nothing): nothing is written
        assert got["text"] == bytes([F.SENTINEL]) * len(text)


def test_a_buffer_one_byte_short_is_reported_with_the_exact_total(exe):
    cs = [c for c in CASES if c["status"] == F.ST_OK and len(ref_of(c)[0]) > 0][::7]
    for c, got in zip(cs, run_cases(exe, cs, [cap_of(c) - 1 for c in cs])):
        text, seg_off = ref_of(c)
        assert got["guards"] == 1 and got["status"] == F.ST_TOO_SMALL and got["total"] == len(text), c["name"]
        assert np.array_equal(got["seg_off"], seg_off) and got["text"] == bytes([F.SENTINEL]) * (len(text) - 1), c["name"]


def test_a_declined_value_wins_over_a_small_buffer(exe):
    cs = [c for c in CASES if c["status"] == F.ST_VALUE]
    for c, got in zip(cs, run_cases(exe, cs, [5] * len(cs))):
        assert got["status"] == F.ST_VALUE and got["declined"] == c["declined"], c["name"]


def test_rounding_equals_bcio_fmt_pyround_float(exe):
    from basecount_amd import _native

    _native.bcio()  # (builds nothing: the library must be there)
    lib = os.path.join(REPO, "basecount_amd", "libbcio.so")
    r = subprocess.run([exe, "sweep", lib], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.startswith("ok ")


def test_the_cases_cover_what_they_are_named_for():
    by = {c["name"]: c for c in CASES}
    starts = set()
    for ln in range(1, 10):
        text = ref_of(by["name%d" % ln])[0]
        at = 0
        for line in text.split(b"\n")[:-1]:
            starts.add(at % 16)
            at += len(line) + 1
    assert starts == set(range(16))
    assert b"\t10737418235\t" in ref_of(by["int32_max_wide"])[0]
    assert b"\t-15\t-3\t" in ref_of(by["negative_counts"])[0] and b"\t-0.0\t-0.0\n" in ref_of(by["negative_counts"])[0]
    assert b"ref\t2147483648\t" in ref_of(by["pos0_%d" % (2**31 - 70)])[0]
    assert b"ref\t1000000000\t" in ref_of(by["pos0_999999990"])[0]
    assert ref_of(by["all_zero"])[0].startswith(b"zero\t1\t0\tA\t0\t-1\t1\t1\n")
    assert b"\t100.0\t0.0\t0.0\t0.0\t1\n" in ref_of(by["all_nz1"])[0]
    # tiles whose text needs several windows of the staging area, and a scan with runs of tiles
    per_tile = len(ref_of(by["name255_long"])[0]) * F.TILE // by["name255_long"]["n"]
    assert per_tile > 3 * F.WIN
    assert by["scan_runs"]["n"] > F.TILE * F.SCAN_THREADS
    lens = [s[1] for s in by["segments_pads_wide"]["segs"]]
    assert 0 in lens and 1 in lens and any(seg[0] % F.TILE == 0 for seg in by["segments_pads_wide"]["segs"])
    assert len(by["segments_40"]["segs"]) == 40
