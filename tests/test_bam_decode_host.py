"""The BAM record decoder (basecount_amd/csrc/bc_bam.h) compiled for the host with AddressSanitizer
and UBSan, as a stand-alone program (tests/native/bamdecode_check.cpp): the speculation, the
stitch, the repair and the fill the device kernels run, as plain loops over the same functions.
Every array must equal the host decoder's (bcio), bit for bit, with 64 guard bytes around the
input and every output, at seg_bytes 256, 1024 and the default and max_records 1, 3 and no limit."""
import os
import subprocess
import tempfile

import pytest

import bam_decode_inputs as B

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seg_bytes, max_records, trunc, final, want_qual)
VALID_CONFIGS = [(seg, lim, 0, 1, 1) for seg in B.SEGS for lim in B.LIMITS] + [(1024, -1, 0, 1, 0), (256, -1, 0, 0, 1)]
PARTIAL_CONFIGS = [(seg, lim, 5, 0, 1) for seg in B.SEGS for lim in (3, -1)]  # the last record cut: not final
REFUSAL_CONFIGS = [(seg, lim, 0, 1, 1) for seg in B.SEGS for lim in (3, -1)] + [(256, -1, 0, 0, 1)]


@pytest.fixture(scope="module")
def checker():
    """run(raw, first, n_refs, configs) -> one result per configuration."""
    src = os.path.join(REPO, "tests", "native", "bamdecode_check.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bamdecode_check")
        try:
            subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas",
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                            os.path.join(REPO, "basecount_amd", "csrc"), src, "-o", exe],
                           check=True, capture_output=True, text=True)
        except FileNotFoundError:
            pytest.skip("no g++")
        except subprocess.CalledProcessError as e:
            raise AssertionError("bamdecode_check.cpp does not compile:\n" + e.stderr)

        def run(raw, first, n_refs, configs):
            vin, vout = os.path.join(tmp, "input.bin"), os.path.join(tmp, "results.bin")
            with open(vin, "wb") as f:
                f.write(B.pack_input(raw, first, n_refs, configs))
            r = subprocess.run([exe, vin, vout], capture_output=True, text=True, timeout=300)
            # the sanitizers stay silent: a report goes to stderr and ends the program non-zero
            assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
            assert r.stdout.startswith("ok %d configurations" % len(configs))
            with open(vout, "rb") as f:
                return B.unpack_results(f.read(), configs)

        yield run


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """The layout and trap files: builder, path, inflated bytes and the host decoder's arrays."""
    d = tmp_path_factory.mktemp("bamdecode")
    out = {}
    lay = B.layout_builder()
    trap, trap_rec = B.trap_builder()
    for name, b in (("layout", lay), ("trap", trap)):
        path = str(d / (name + ".bam"))
        B.write_bam(path, b)
        out[name] = dict(builder=b, path=path, raw=b.raw(), exp=B.host_arrays(path))
    out["trap"]["rec"] = trap_rec
    return out


def _check_valid(checker, raw, exp, name):
    first, n_refs = B.header_info(raw)
    res = checker(raw, first, n_refs, VALID_CONFIGS)
    for c, r in zip(VALID_CONFIGS, res):
        what = "%s seg_bytes=%d max_records=%d final=%d" % (name, c[0], c[1], c[3])
        assert r["guards"] == 1, what
        assert r["status"] == 0, "%s: declined, status %d at %d" % (what, r["status"], r["err_off"])
        assert r["used"] == len(raw), what
        B.assert_arrays_equal(r, exp, bool(c[4]), what)
        if c[1] > 0:
            assert r["batches"] >= min(exp["n"] // c[1], 32), what  # the cut really cut
    return res


@pytest.mark.parametrize("name", sorted(B.GOLDEN_BAMS))
def test_golden_files_decode_to_the_host_decoders_arrays(checker, name):
    path = os.path.join(B.GOLDEN, B.GOLDEN_BAMS[name])
    _check_valid(checker, B.inflated(path), B.host_arrays(path), name)


def test_layout_file_decodes_to_the_host_decoders_arrays(checker, synthetic):
    s = synthetic["layout"]
    assert s["exp"]["n"] == len(s["builder"].recs)
    _check_valid(checker, s["raw"], s["exp"], "layout")


def test_partial_last_record_waits_for_more_bytes(checker, synthetic):
    s = synthetic["layout"]
    b, raw = s["builder"], s["raw"]
    assert 0 < 5 < b.ends[-1] - b.starts[-1]
    first, n_refs = B.header_info(raw)
    exp = B.first_records(s["exp"], s["exp"]["n"] - 1)
    for c, r in zip(PARTIAL_CONFIGS, checker(raw, first, n_refs, PARTIAL_CONFIGS)):
        what = "partial seg_bytes=%d max_records=%d" % (c[0], c[1])
        assert r["guards"] == 1 and r["status"] == 0, what
        assert r["used"] == b.starts[-1], what
        B.assert_arrays_equal(r, exp, True, what)


def test_trap_records_inside_a_qual_field_are_not_believed(checker, synthetic):
    s = synthetic["trap"]
    res = _check_valid(checker, s["raw"], s["exp"], "trap")
    by_config = dict(zip(VALID_CONFIGS, res))
    # at 1024 the segment behind the field starts inside it: its speculated entry is a copied record
    assert by_config[(1024, -1, 0, 1, 1)]["repaired"] >= 1


@pytest.mark.parametrize("name", sorted(B.refusals()))
def test_rule_violations_decline_where_the_host_decoder_fails(checker, name, tmp_path):
    from basecount_amd.bam import BamFile

    raw, msg = B.refusals()[name]
    path = str(tmp_path / "bad.bam")
    with open(path, "wb") as f:
        f.write(B.bgzf(raw))
    with pytest.raises(Exception) as ei:  # the host decoder's own message
        BamFile(path)
    assert msg in str(ei.value), str(ei.value)
    first, n_refs = B.header_info(raw)
    for c, r in zip(REFUSAL_CONFIGS, checker(raw, first, n_refs, REFUSAL_CONFIGS)):
        what = "%s seg_bytes=%d max_records=%d final=%d" % (name, c[0], c[1], c[3])
        assert r["guards"] == 1, what
        partial_ok = c[3] == 0 and name in ("truncated_last_record", "ends_in_length_prefix")
        if partial_ok:  # more bytes may follow: the complete records, no refusal
            assert r["status"] == 0 and r["n"] == 9, what
        else:
            assert r["status"] != 0 and B.STATUS_MESSAGE[r["status"]] == msg, "%s: status %d" % (what, r["status"])
