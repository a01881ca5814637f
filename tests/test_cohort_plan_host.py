"""plan_cohort (basecount_amd/cohort.py): a pure function from per-file facts to the launches of a
cohort.  No device and no file: the sizes that reach the 2^32 budgets are synthetic numbers."""
import os

import pytest

from basecount_amd import cohort as Co

F = Co.FileFacts
CAP, BUDGET = 1 << 24, 1 << 30


def reg(path, lengths=(30_000,), n_reads=4_000, cig_words=4_100, seq_bytes=300_000, ops=False):
    return F(path, None, tuple(lengths), n_reads, cig_words, seq_bytes, ops)


def plan(facts, cap=CAP, budget=BUDGET, want_qual=False):
    groups, single = Co.plan_cohort(facts, cap, budget, want_qual)
    return [[f.path for f in g] for g in groups], [(f.path, r) for f, r in single]


def test_consecutive_regular_files_are_one_group_in_input_order():
    groups, single = plan([reg(p) for p in "dcba"])
    assert groups == [list("dcba")] and single == []


def test_cut_at_the_position_cap():
    # round_up(30000, 64) = 30016: three files fit 90048 positions, the fourth does not
    groups, single = plan([reg(p) for p in "abcdefg"], cap=3 * 30016)
    assert groups == [list("abc"), list("def")] and single == [("g", "lone segment")]
    groups, _ = plan([reg(p) for p in "abcdef"], cap=3 * 30016 - 1)
    assert groups == [list("ab"), list("cd"), list("ef")]
    # the pad counts: 65 positions take 128
    groups, _ = plan([reg(p, lengths=(65,)) for p in "abcd"], cap=256)
    assert groups == [list("ab"), list("cd")]


def test_a_file_larger_than_the_cap_is_single_and_splits_the_run():
    groups, single = plan([reg("a"), reg("b"), reg("big", lengths=(100_000,)), reg("c"), reg("d")], cap=70_000)
    assert groups == [["a", "b"], ["c", "d"]]
    assert single == [("big", "exceeds the group's position cap")]


def test_cut_at_the_cigar_word_budget():
    half = 1 << 31
    # 2^31 + (2^31 - 1) = 2^32 - 1 words fit; one more reaches 2^32
    groups, _ = plan([reg("a", cig_words=half), reg("b", cig_words=half - 1), reg("c"), reg("d")], budget=1 << 62)
    assert groups == [["a", "b"], ["c", "d"]]  # a + b + c would reach 2^32
    groups, single = plan([reg("a", cig_words=half), reg("b", cig_words=half), reg("c")], budget=1 << 62)
    assert groups == [["b", "c"]] and single == [("a", "lone segment")]
    _, single = plan([reg("a", cig_words=1 << 32), reg("b")], budget=1 << 62)
    assert single[0] == ("a", "exceeds the 32-bit index budgets")


def test_cut_at_the_nibble_budget():
    q = 1 << 30  # bytes: 2 x (2^30 + 2^30) nibbles = 2^32
    groups, single = plan([reg("a", seq_bytes=q), reg("b", seq_bytes=q), reg("c", seq_bytes=16)], budget=1 << 62)
    assert groups == [["b", "c"]] and single == [("a", "lone segment")]
    groups, _ = plan([reg("a", seq_bytes=q), reg("b", seq_bytes=q - 16)], budget=1 << 62)
    assert groups == [["a", "b"]]  # 2^32 - 32 nibbles
    _, single = plan([reg("a", seq_bytes=1 << 31)], budget=1 << 62)
    assert single == [("a", "exceeds the 32-bit index budgets")]


def test_cut_at_the_read_budget():
    h = 1 << 30
    groups, single = plan([reg("a", n_reads=h), reg("b", n_reads=h), reg("c", n_reads=h - 1)], budget=1 << 62)
    assert groups == [["b", "c"]] and single == [("a", "lone segment")]


def test_cut_at_the_byte_budget_and_qualities_count():
    f = reg("x")
    assert f.upload_bytes(False) == 4 * 4_100 + 300_000 + 16 * 4_000
    assert f.upload_bytes(True) == f.upload_bytes(False) + 2 * 300_000
    one = f.upload_bytes(False)
    groups, _ = plan([reg(p) for p in "abcd"], budget=2 * one)
    assert groups == [["a", "b"], ["c", "d"]]
    groups, _ = plan([reg(p) for p in "abcd"], budget=4 * one)
    assert groups == [list("abcd")]
    # with qualities the same budget holds fewer files
    two_q = 2 * f.upload_bytes(True)
    assert plan([reg(p) for p in "abcd"], budget=two_q)[0] == [list("abcd")]
    groups, single = plan([reg(p) for p in "abcd"], budget=two_q, want_qual=True)
    assert groups == [["a", "b"], ["c", "d"]] and single == []
    _, single = plan([reg("a"), reg("b")], budget=one - 1)
    assert [r for _, r in single] == ["exceeds the upload budget"] * 2


def test_cut_at_an_ops_boundary():
    groups, single = plan([reg("a"), reg("b"), reg("o1", ops=True), reg("o2", ops=True), reg("c")])
    assert groups == [["a", "b"], ["o1", "o2"]] and single == [("c", "lone segment")]


def test_an_irregular_file_ends_a_run():
    groups, single = plan([reg("a"), reg("b"), F("bad", "unsorted within a reference"), reg("c"), reg("d"),
                           F("worse", "a read outside its reference"), reg("e")])
    assert groups == [["a", "b"], ["c", "d"]]
    assert single == [("bad", "unsorted within a reference"), ("worse", "a read outside its reference"),
                      ("e", "lone segment")]


def test_a_lone_segment_is_single_and_a_lone_two_reference_file_is_a_group():
    assert plan([reg("a")]) == ([], [("a", "lone segment")])
    assert plan([reg("a", lengths=(3_000, 3_200))]) == ([["a"]], [])
    groups, single = plan([F("x", "no records"), reg("a", lengths=(3_000, 3_200)), F("y", "no records"), reg("b")])
    assert groups == [["a"]] and single == [("x", "no records"), ("y", "no records"), ("b", "lone segment")]
    assert plan([reg("a", lengths=())]) == ([], [("a", "no requested reference")])


def test_grouping_off_makes_every_file_single(monkeypatch):
    assert plan([reg("a"), reg("b")], cap=0) == ([], [("a", "grouping is off"), ("b", "grouping is off")])
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "0")
    groups, single = Co.plan_cohort([reg("a"), reg("b")])
    assert groups == [] and len(single) == 2


def test_the_defaults_come_from_the_environment(monkeypatch):
    monkeypatch.delenv("BASECOUNT_GROUP_REFS", raising=False)
    monkeypatch.setenv("BASECOUNT_GROUP_MAX", str(2 * 30016))
    monkeypatch.setenv("BASECOUNT_COHORT_BYTES", str(1 << 40))
    groups, _ = Co.plan_cohort([reg(p) for p in "abcd"])
    assert [[f.path for f in g] for g in groups] == [["a", "b"], ["c", "d"]]
    monkeypatch.delenv("BASECOUNT_GROUP_MAX")
    monkeypatch.setenv("BASECOUNT_COHORT_BYTES", str(2 * reg("a").upload_bytes(False)))
    groups, _ = Co.plan_cohort([reg(p) for p in "abcd"])
    assert [[f.path for f in g] for g in groups] == [["a", "b"], ["c", "d"]]
    monkeypatch.delenv("BASECOUNT_COHORT_BYTES")
    assert Co.byte_budget() == 1 << 30 and Co.thread_budget() == 16
    monkeypatch.setenv("BASECOUNT_COHORT_THREADS", "3")
    assert Co.thread_budget() == 3


def test_the_incremental_planner_is_the_pure_function():
    """The decoder feeds Planner.add file by file; the units it closes are plan_cohort's, in order."""
    facts = [reg("a"), reg("b"), F("bad", "no records"), reg("o", ops=True), reg("c"), reg("d", lengths=(5, 6))]
    p = Co.Planner(CAP, BUDGET, False)
    closed_at = [[(u[0], [f.path for f in u[1]] if u[0] == "group" else u[1].path) for u in p.add(f)] for f in facts]
    assert closed_at == [[], [], [("group", ["a", "b"]), ("single", "bad")], [], [("single", "o")], []]
    assert [(u[0], [f.path for f in u[1]]) for u in p.finish()] == [("group", ["c", "d"])]


def test_output_naming_and_duplicate_basenames():
    names = Co.output_names(["/data/run1/s1.bam", "s2.sorted.bam", "dir/s3"], "out")
    assert names == [os.path.join("out", "s1.tsv"), os.path.join("out", "s2.sorted.tsv"), os.path.join("out", "s3.tsv")]
    with pytest.raises(ValueError) as ei:
        Co.output_names(["a/s1.bam", "b/s2.bam", "c/s1.bam"], "out")
    assert "s1" in str(ei.value) and "a/s1.bam" in str(ei.value) and "c/s1.bam" in str(ei.value)


def test_the_command_refuses_duplicates_and_several_ranks_before_any_work(tmp_path, monkeypatch, capsys):
    out = tmp_path / "o"
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert Co.run(["--out-dir", str(out), "a/s1.bam", "b/s1.bam"]) == 2
    assert "duplicate basename" in capsys.readouterr().err and not out.exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert Co.run(["--out-dir", str(out), "a/s1.bam"]) == 2
    assert "WORLD_SIZE" in capsys.readouterr().err and not out.exists()
    monkeypatch.delenv("WORLD_SIZE")
    lst = tmp_path / "list.txt"
    lst.write_text("x/s1.bam\n\n  y/s1.bam  \n")
    assert Co.run(["--out-dir", str(out), "--bam-list", str(lst)]) == 2
    assert "duplicate basename" in capsys.readouterr().err
    with pytest.raises(SystemExit):  # basecount's own checks: the flags are its parser's
        Co.run(["--out-dir", str(out), "--long-format", "--summarise", "a.bam"])
