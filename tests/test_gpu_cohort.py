"""get_basecounts_many on the GPU: every file's result is what get_basecounts gives for that file in
this process -- the same keys in the same order, the arrays bit for bit, the same exception -- and
cohort.PLAN shows the routing: consecutive regular files in one launch, the irregular ones through
the per-file path with their reasons.

Inputs, in this order: c1, mixed, a copy of c1 under another name, ont (two references, long reads),
edge (unsorted within its references), err_range (a read outside its reference)."""
import os
import shutil

import numpy as np
import pytest

from basecount_amd import cohort as Co
from basecount_amd import main as M
from basecount_amd.scheme import load_scheme

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENV = ("BASECOUNT_GROUP_MAX", "BASECOUNT_GROUP_REFS", "BASECOUNT_LONG_READS", "BASECOUNT_DEVICE_FORMAT",
       "BASECOUNT_BATCH_RECORDS", "BASECOUNT_COHORT_BYTES", "BASECOUNT_DEVICE_INFLATE", "BASECOUNT_DEVICE_DECODE",
       "BASECOUNT_DEVICE_SELECT")


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    copy = str(tmp_path_factory.mktemp("cohort") / "c1_again.bam")
    shutil.copyfile(os.path.join(GOLDEN, "c1.bam"), copy)
    return [os.path.join(GOLDEN, "c1.bam"), os.path.join(GOLDEN, "mixed.bam"), copy,
            os.path.join(GOLDEN, "ont", "ont.bam"), os.path.join(GOLDEN, "edge.bam"),
            os.path.join(GOLDEN, "err_range.bam")]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


WINDOWS = [(t[2]["inside_start"], t[2]["inside_end"]) for t in load_scheme(os.path.join(GOLDEN, "scheme.bed"))]


def _tiles(ref):
    return WINDOWS


MODES = {
    "rows": dict(),
    "rows_n": dict(show_n_bases=True),
    "long": dict(long_format=True),
    "long_n": dict(show_n_bases=True, long_format=True),
    "summary": dict(_mode="summary"),
    "bed": dict(_mode="summary", _tiles=_tiles),
}


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_result(got, exp, what):
    """One file's result against get_basecounts' (or the exception it raised)."""
    if isinstance(exp, BaseException):
        assert type(got) is type(exp) and str(got) == str(exp), (what, got, exp)
        return
    assert not isinstance(got, BaseException), (what, got)
    assert list(got) == list(exp), what  # the same references in the same (set) order
    for ref in exp:
        g, e = got[ref], exp[ref]
        assert list(g) == list(e) and g["num_reads"] == e["num_reads"], (what, ref)
        if "rows" in e:
            assert (g["rows"].ref, g["rows"].long, g["rows"].k) == (e["rows"].ref, e["rows"].long, e["rows"].k)
            for name in ("counts", "pc", "ent", "sec", "cov"):
                assert _same_bits(getattr(g["rows"].d, name), getattr(e["rows"].d, name)), (what, ref, name)
        elif "text" in e:
            assert bytes(g["text"]) == bytes(e["text"]), (what, ref)
        else:
            assert g["length"] == e["length"] and list(g["summary"]) == list(e["summary"]), (what, ref)
            for name, v in e["summary"].items():
                if name == "amplicons":
                    assert _same_bits(g["summary"][name][0], v[0]), (what, ref)
                    assert list(g["summary"][name][1]) == list(v[1]), (what, ref)
                else:
                    assert type(g["summary"][name]) is type(v) and _same_bits(g["summary"][name], v), (what, ref, name)


def _per_file(bams, **kw):
    out = {}
    for b in bams:
        try:
            out[b] = M.get_basecounts(b, **kw)
        except Exception as e:  # noqa: BLE001 - the file's expected result
            out[b] = e
    return out


def _check(bams, **kw):
    got = Co.get_basecounts_many(bams, **kw)
    plan = {k: list(v) for k, v in Co.PLAN.items()}
    exp = _per_file(bams, **kw)
    assert list(got) == list(bams)
    for b in bams:
        assert_same_result(got[b], exp[b], os.path.basename(b))
    return got, plan


def _default_plan(bams):
    c1, mixed, again, ont, edge, bad = bams
    return {"groups": [[(c1, "ref"), (mixed, "MN908947.3"), (again, "ref")], [(ont, "ontA"), (ont, "ontB")]],
            "single": [(edge, "unsorted within a reference"), (bad, "a read outside its reference")],
            "ops": [[(ont, "ontA"), (ont, "ontB")]]}


@pytest.mark.parametrize("mbq,mmq", [(0, 0), (20, 30)])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_file_equals_get_basecounts(bams, mode, mbq, mmq):
    got, plan = _check(bams, min_base_quality=mbq, min_mapping_quality=mmq, **MODES[mode])
    assert plan == _default_plan(bams)
    bad = got[bams[5]]
    if mbq == 0:  # (at 20 the overhanging base is below the quality bar: the file then simply succeeds)
        assert type(bad) is IndexError
        assert str(bad) == "vector::_M_range_check: __n (which is 60) >= this->size() (which is 60)"
    assert not isinstance(got[bams[4]], BaseException) and len(got[bams[4]]) == 4  # edge: all four references
    if mode == "bed":
        amp, empty = got[bams[1]]["MN908947.3"]["summary"]["amplicons"]
        assert amp.shape == (len(WINDOWS), 6) and not any(empty) and len(WINDOWS) > 10
        # c1's reference ends before the scheme does: its own clip decides which windows are empty
        assert any(got[bams[0]]["ref"]["summary"]["amplicons"][1])


@pytest.mark.parametrize("mode", ["rows", "bed"])
def test_a_smaller_cap_makes_mixed_single_and_splits_the_run(bams, monkeypatch, mode):
    monkeypatch.setenv("BASECOUNT_GROUP_MAX", "16384")
    _, plan = _check(bams, min_base_quality=20, **MODES[mode])
    c1, mixed, again, ont, edge, bad = bams
    assert plan["groups"] == [[(ont, "ontA"), (ont, "ontB")]] == plan["ops"]
    assert plan["single"] == [(c1, "lone segment"), (mixed, "exceeds the group's position cap"),
                              (again, "lone segment"), (edge, "unsorted within a reference"),
                              (bad, "a read outside its reference")]


@pytest.mark.parametrize("mode", ["rows", "summary"])
def test_grouping_off_makes_every_file_single(bams, monkeypatch, mode):
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "0")
    _, plan = _check(bams, **MODES[mode])
    assert plan["groups"] == [] and plan["ops"] == []
    assert plan["single"] == [(b, "grouping is off") for b in bams]


@pytest.mark.parametrize("mode", ["long_n", "bed"])
def test_long_read_routing_forced_on_is_one_group_on_the_long_read_shape(bams, monkeypatch, mode):
    monkeypatch.setenv("BASECOUNT_LONG_READS", "1")
    _, plan = _check(bams, min_base_quality=20, min_mapping_quality=30, **MODES[mode])
    exp = _default_plan(bams)
    group = exp["groups"][0] + exp["groups"][1]  # every file wants the same shape now: nothing cuts the run
    assert plan["groups"] == [group] and plan["ops"] == [group] and plan["single"] == exp["single"]


def test_small_upload_budget_cuts_groups_and_results_stay(bams, monkeypatch):
    """c1 and mixed upload 95,024 + 438,544 bytes; the copy of c1 would pass 540,000 with them."""
    monkeypatch.setenv("BASECOUNT_COHORT_BYTES", "540000")
    _, plan = _check(bams[:4])
    c1, mixed, again, ont = bams[:4]
    assert plan["groups"] == [[(c1, "ref"), (mixed, "MN908947.3")], [(ont, "ontA"), (ont, "ontB")]]
    assert plan["single"] == [(again, "lone segment")]


def test_device_formatted_text_equals_the_per_file_text(bams):
    got, plan = _check(bams, _mode="text", _dp=3)
    assert plan == _default_plan(bams)
    assert bytes(got[bams[0]]["ref"]["text"]).startswith(b"ref\t1\t")


def test_a_bed_that_does_not_load_sends_every_file_through_the_per_file_path(bams):
    def broken(ref):
        return None

    got = Co.get_basecounts_many(bams[:3], _mode="summary", _tiles=broken)
    assert Co.PLAN["groups"] == [] and [r for _, r in Co.PLAN["single"]] == ["the BED file does not load"] * 3
    exp = _per_file(bams[:3], _mode="summary", _tiles=broken)
    for b in bams[:3]:
        assert_same_result(got[b], exp[b], b)


def test_a_requested_reference_subset_and_a_missing_file(bams, tmp_path):
    missing = str(tmp_path / "nope.bam")
    files = [bams[3], missing, bams[0]]
    got = Co.get_basecounts_many(files, references=["ontB"])
    exp = _per_file(files, references=["ontB"])
    for b in dict.fromkeys(files):
        assert_same_result(got[b], exp[b], b)
    assert type(got[missing]) is FileNotFoundError
    assert type(got[bams[0]]) is Exception and "not a valid reference" in str(got[bams[0]])
    assert Co.PLAN["groups"] == []  # ont with one requested reference is a lone segment
