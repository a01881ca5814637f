"""BASECOUNT_DEVICE_FORMAT=1 end to end: run() with the rows written on the device against the
reference's goldens (tests/golden/) and against the default path, byte for byte: wide rows, long
format, --show-n-bases, decimal places 0 .. 4; the decimal places the kernels do not cover, where the
host formatter is used; the accumulate path (BASECOUNT_BATCH_RECORDS=3); and a grouped file of 40
small references, some without reads.  main.PLAN["format"] must show that the device path was in
fact taken where it should be."""
import contextlib
import gzip
import io
import os

import numpy as np
import pytest

import oracle as O
from basecount_amd import main, synth

pytestmark = pytest.mark.gpu

SWITCH = "BASECOUNT_DEVICE_FORMAT"


def run_cli(argv):
    buf = io.BytesIO()
    txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
    with contextlib.redirect_stdout(txt):
        main.run(argv)
        txt.flush()
    return buf.getvalue()


@pytest.fixture
def in_golden(golden, monkeypatch):
    monkeypatch.chdir(golden)
    for k in (SWITCH, "BASECOUNT_BATCH_RECORDS", "BASECOUNT_DEVICE_SELECT", "BASECOUNT_DEVICE_DECODE",
              "BASECOUNT_DEVICE_INFLATE", "BASECOUNT_GROUP_REFS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def on_and_off(mp, argv):
    """(output with the switch on, PLAN["format"] of that run, output with it off)."""
    mp.setenv(SWITCH, "1")
    on = run_cli(argv)
    plan = main.PLAN.get("format")
    mp.delenv(SWITCH)
    off = run_cli(argv)
    assert main.PLAN.get("format") is None  # the switch off: nothing recorded
    return on, plan, off


def golden_text(c):
    with open(c["stdout"], "rb") as fh:
        return gzip.decompress(fh.read())


def assert_golden(got, c):
    exp = golden_text(c)
    h1, b1 = O.split_blocks(got.decode(), False)
    h2, b2 = O.split_blocks(exp.decode(), False)
    assert h1 == h2 and b1 == b2  # (several references: the set order is the process's)
    if len(b2) == 1:
        assert got == exp


COVERED = ["c1_default", "c1_long", "c1_shown", "c1_q20_m30", "edge_default_h1", "edge_long", "edge_long_shown_dp0",
           "edge_chunk3", "edge_refs_all", "edge_q20_m30", "edge_q40_m60_wide5", "mixed_default", "mixed_shown_long",
           "mixed_q20_m30", "err_range_q20"]
NOT_COVERED = ["c1_dp5", "edge_dp17_shown", "edge_long_dp17", "mixed_dp17"]


@pytest.mark.parametrize("name", COVERED)
@pytest.mark.parametrize("batch", [None, "3"])
def test_goldens_with_the_rows_written_on_the_device(in_golden, manifest, name, batch):
    c = manifest[name]
    if batch:
        in_golden.setenv("BASECOUNT_BATCH_RECORDS", batch)  # every reference accumulated over many batches
    on, plan, off = on_and_off(in_golden, [c["bam"]] + c["args"])
    assert on == off
    assert_golden(on, c)
    nrefs = len(O.split_blocks(on.decode(), False)[1])
    assert plan == {"device": nrefs, "host": 0, "declined": []}


@pytest.mark.parametrize("name", NOT_COVERED)
@pytest.mark.parametrize("batch", [None, "3"])
def test_uncovered_decimal_places_use_the_host_formatter(in_golden, manifest, name, batch):
    c = manifest[name]
    if batch:
        in_golden.setenv("BASECOUNT_BATCH_RECORDS", batch)
    on, plan, off = on_and_off(in_golden, [c["bam"]] + c["args"])
    assert on == off
    assert_golden(on, c)
    assert plan["device"] == 0 and plan["host"] >= 1 and plan["declined"] == []


def test_summaries_are_untouched(in_golden, manifest):
    for name in ("mixed_bed_dp16", "c1_summary"):
        c = manifest[name]
        in_golden.setenv(SWITCH, "1")
        got = run_cli([c["bam"]] + c["args"])
        assert main.PLAN.get("format") is None
        assert O.split_blocks(got.decode(), True) == O.split_blocks(golden_text(c).decode(), True)


@pytest.mark.parametrize("dp", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("shape", [[], ["--long-format"], ["--show-n-bases"], ["--long-format", "--show-n-bases"]])
def test_every_decimal_place_and_shape(in_golden, dp, shape):
    on, plan, off = on_and_off(in_golden, ["mixed.bam", "--decimal-places", str(dp)] + shape)
    assert on == off and len(on) > 1000
    assert plan["device"] >= 1 and plan["host"] == 0 and plan["declined"] == []


@pytest.fixture(scope="module")
def forty_refs(tmp_path_factory):
    rng = np.random.default_rng(40)
    contigs = [("contig%02d" % i, int(L)) for i, L in enumerate(rng.integers(1, 301, 40))]
    contigs[7] = ("contig07", 1)
    contigs[8] = ("contig08", 300)
    path = str(tmp_path_factory.mktemp("fmt_cli") / "refs40.bam")
    rs = synth.make_reads(contigs, 6, mixed=True, seed=41, read_len=24)
    lens = np.asarray([L for _, L in contigs])
    keep = np.flatnonzero(lens[rs.tid] >= 40)  # the shorter references stay without reads
    assert 0 < keep.size < rs.n
    synth.write_bam(synth.subset(rs, keep), path)
    return path, contigs


@pytest.mark.parametrize("shape", [[], ["--long-format", "--show-n-bases", "--decimal-places", "2"]])
def test_forty_small_references_take_the_grouped_path(in_golden, forty_refs, shape):
    path, contigs = forty_refs
    on, plan, off = on_and_off(in_golden, [path] + shape)
    assert on == off
    blocks = O.split_blocks(on.decode(), False)[1]
    assert len(blocks) == 40
    k = 6 if shape else 1
    assert {n: b.count("\n") for n, b in blocks.items()} == {n: L * k for n, L in contigs}
    if not shape:  # a reference of one position, without reads
        assert blocks["contig07"] == "contig07\t1\t0\t0\t0\t0\t0\t0\t-1\t-1\t-1\t-1\t-1\t1\t1\n"
    assert sum(len(g) for g in main.PLAN["groups"]) >= 30
    assert plan == {"device": 40, "host": 0, "declined": []}


def test_a_small_estimate_is_repeated_once_at_the_exact_size(in_golden, forty_refs):
    in_golden.setattr(main._DeviceFormatter, "_estimate", lambda self, segs, n: 16)
    before = main._FORMAT_MS["retries"]
    for argv in (["mixed.bam", "--long-format"], [forty_refs[0]]):
        main.release_device_memory()  # (a text buffer kept from an earlier run would be large enough)
        on, plan, off = on_and_off(in_golden, argv)
        assert on == off and plan["host"] == 0 and plan["declined"] == []
    assert main._FORMAT_MS["retries"] >= before + 2


def test_references_and_groups_in_slices(in_golden, forty_refs):
    """A reference above FORMAT_SLICE positions goes through in slices (pos0), a group in runs of
    segments of at most that span."""
    in_golden.setattr(main, "FORMAT_SLICE", 320)
    for argv, ngroups in ((["mixed.bam"], 0), (["c1.bam", "--long-format", "--show-n-bases"], 0), ([forty_refs[0]], 1)):
        on, plan, off = on_and_off(in_golden, argv)
        assert on == off and plan["device"] >= 1 and plan["host"] == 0 and plan["declined"] == []
        assert len(main.PLAN["groups"]) >= ngroups


def test_a_declined_value_falls_back_to_the_host_formatter(in_golden):
    """BC_FMT_VALUE (a printed value that is not finite): _collect downloads the arrays as ever and
    the reference is named in PLAN["format"]["declined"]."""
    from basecount_amd import device as D

    ctx = main.context()
    scratch = main._Scratch(ctx)
    L, k = 200, 5
    rng = np.random.default_rng(7)
    counts = rng.integers(1, 50, (k, L)).astype(np.int32)
    pc = counts / counts.sum(0) * 100
    ent, sec = rng.random(L), rng.random(L)
    ent[131] = np.nan
    hist = scratch.get("hist", counts.nbytes).upload(counts)
    outs = scratch.outputs(k, L, want_pc=True)
    outs["pc"].upload(pc)
    outs["ent"].upload(ent)
    outs["sec"].upload(sec)
    outs["cov"].upload(counts.sum(0).astype(np.int32))
    main.PLAN["format"] = {"device": 0, "host": 0, "declined": []}
    try:
        fm = scratch.formatter = main._DeviceFormatter(ctx, scratch, k, 3, False)
        fm.name = "nanref"
        d = main._collect(ctx, outs, hist, L, k, k, "rows", None, False, scratch, stats_done=True)
        assert isinstance(d, main.RefData) and np.array_equal(d.counts, counts) and np.isnan(d.ent[131])
        assert main.PLAN["format"]["declined"] == ["nanref"]
        ent[131] = 0.5
        outs["ent"].upload(ent)
        text = main._collect(ctx, outs, hist, L, k, k, "rows", None, False, scratch, stats_done=True)
        from basecount_amd import fmt

        assert bytes(text) == fmt.rows_text("nanref", counts, pc, ent, sec, 3, False)
        assert D.FMT_STATUS[D.FMT_VALUE] == "value"
    finally:
        ctx.sync()
        scratch.release()
        main.PLAN.pop("format", None)


def test_the_timing_report_names_the_formatter(in_golden, capfd):
    in_golden.setenv(SWITCH, "1")
    in_golden.setenv("BASECOUNT_HIP_TIMING", "1")
    try:
        run_cli(["c1.bam"])
    finally:
        main.context().timing(False)
    err = capfd.readouterr().err
    assert "device format:" in err and "k_fmt_measure + k_fmt_scan + k_fmt_write" in err and "text download" in err


def test_errors_surface_where_they_did(in_golden, manifest):
    """A failing file fails the same, before the first byte is written."""
    for name in ("err_range", "err_nocigar"):
        c = manifest[name]
        lines = []
        for sw in ("1", None):
            if sw:
                in_golden.setenv(SWITCH, sw)
            else:
                in_golden.delenv(SWITCH)
            buf = io.BytesIO()
            txt = io.TextIOWrapper(buf, encoding="utf-8", write_through=True)
            with contextlib.redirect_stdout(txt), pytest.raises(BaseException) as ei:
                main.run([c["bam"]] + c["args"])
            txt.flush()
            assert buf.getvalue() == b""
            lines.append(f"{type(ei.value).__name__}: {ei.value}".splitlines()[0])
        assert lines[0] == lines[1] == c["error"]
