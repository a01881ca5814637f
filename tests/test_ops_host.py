"""Host side of the long-read kernel shape ("ops", DESIGN.md §3 "k_ops"): the shape's id, the
nanopore-like read generator, the routing rule and the reference-made ``ont`` goldens.  No GPU."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import oracle as O
from basecount_amd import device as D
from basecount_amd import main as M
from basecount_amd import synth
from basecount_amd.bam import BamFile

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ONT = os.path.join(GOLDEN, "ont")
CONTIGS = [("a", 6000), ("b", 2500)]
REF_OPS, QUERY_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8)


def per_read(rs, ops):
    """Sum of the lengths of the given CIGAR ops, per read."""
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    rec = np.repeat(np.arange(rs.n), n_ops)
    ln = np.where(np.isin(rs.cigar & 15, ops), rs.cigar >> 4, 0).astype(np.int64)
    return np.bincount(rec, ln, rs.n).astype(np.int64)


def test_shape_id():
    assert D.SHAPES["ops"] == 4
    assert sorted(D.SHAPES.values()) == list(range(5))


def test_make_long_reads_deterministic_per_seed():
    a = synth.make_long_reads(CONTIGS, 200, seed=3)
    b = synth.make_long_reads(CONTIGS, 200, seed=3)
    c = synth.make_long_reads(CONTIGS, 200, seed=4)
    for f in ("tid", "pos", "mapq", "cig_off", "cigar", "l_seq", "seq_off", "seq", "qual", "qstart"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert not np.array_equal(a.cigar, c.cigar)


@pytest.mark.parametrize("unsorted", [False, True])
def test_make_long_reads_cigars_are_valid(unsorted):
    rs = synth.make_long_reads(CONTIGS, 300, seed=5, mean_len=500, indel_every=12, unsorted=unsorted)
    assert rs.n == 600 and rs.references == ["a", "b"] and rs.lengths == [6000, 2500]
    op, ln = rs.cigar & 15, rs.cigar >> 4
    assert np.all(op <= 8) and np.all(ln > 0)
    assert np.array_equal(per_read(rs, QUERY_OPS), rs.l_seq)  # query consumption
    span = per_read(rs, REF_OPS)
    L = np.asarray(rs.lengths)[rs.tid]
    assert np.all(rs.pos >= 0) and np.all(rs.pos + span <= L)
    # H only outermost, S only next to it or at the ends; the leading S is qstart
    beg, end = rs.cig_off[:-1].astype(np.int64), rs.cig_off[1:].astype(np.int64)
    inner = np.ones(rs.cigar.size, bool)
    for k in (0, 1):
        inner[beg + k] = False
        inner[end - 1 - k] = False
    assert not np.any(np.isin(op[inner], (4, 5)))
    lead = np.where(op[beg] == 5, beg + 1, beg)
    assert np.array_equal(np.where(op[lead] == 4, ln[lead], 0), rs.qstart)
    assert {1, 2, 3, 7, 8} <= set(op.tolist())  # I, D, N, = and X all occur
    # per contig in start order unless unsorted
    for t in (0, 1):
        p = rs.pos[rs.tid == t]
        assert bool(np.all(np.diff(p) >= 0)) != unsorted
    # stored bytes and qualities by nibble index
    assert np.all(rs.l_seq % 2 == 0) and np.array_equal(rs.qual_off, 2 * rs.seq_off)
    assert rs.seq.size == int(rs.seq_off[-1]) and rs.qual.size == 2 * rs.seq.size


@pytest.mark.parametrize("mean_len, indel_every, lo, hi", [
    (500, 500, 1.5, 5), (500, 62, 13, 21), (500, 15.6, 55, 75), (500, 7.8, 110, 150), (8000, 15, 900, 1200)])
def test_make_long_reads_ops_regime(mean_len, indel_every, lo, hi):
    """Mean ops per read ~ 2 mean_len / indel_every (+ clips); mean stored length ~ mean_len."""
    rs = synth.make_long_reads([("x", 200_000)], 1500 if mean_len < 1000 else 150, seed=9, mean_len=mean_len,
                               indel_every=indel_every)
    n_ops = np.diff(rs.cig_off.astype(np.int64))
    assert lo <= n_ops.mean() <= hi, n_ops.mean()
    assert 0.8 * mean_len <= rs.l_seq.mean() <= 1.35 * mean_len, rs.l_seq.mean()


def test_make_long_reads_too_long_for_the_contig():
    with pytest.raises(ValueError):
        synth.make_long_reads([("x", 40)], 50, seed=1, mean_len=500)


def test_oracle_counts_long_reads_without_range_error(tmp_path):
    rs = synth.make_long_reads(CONTIGS, 150, seed=6)
    ev = 0
    for t, L in enumerate(rs.lengths):
        b = synth.batch_arrays(rs, t)
        cnt, (bad, _) = O.bcount(L, 0, b)
        assert bad == -1
        ev += int(cnt.sum())
    # every reference event is an A/C/G/T/N base or a deletion
    assert ev == synth.ref_events(rs)
    # and the BAM writer / decoder round trip keeps the records
    path = str(tmp_path / "long.bam")
    synth.write_bam(rs, path)
    with BamFile(path) as f:
        assert f.n_records == rs.n
        assert np.array_equal(f.pos, rs.pos) and np.array_equal(f.cigar, rs.cigar)
        assert np.array_equal(f.seq, rs.seq) and np.array_equal(f.qstart, rs.qstart)


def slices(path):
    """cig_n of every reference's accepted reads of a BAM file."""
    with BamFile(path) as f:
        sel = f.select(0, [True] * len(f.references))
        return [np.array(sel.cig_n[int(sel.ref_beg[t]):int(sel.ref_beg[t + 1])]) for t in range(len(f.references))]


def test_wants_ops_rule(monkeypatch):
    monkeypatch.delenv("BASECOUNT_LONG_READS", raising=False)
    monkeypatch.setattr(M, "OPS_RULE_DEFAULT", True)  # the rule itself, whatever the shipped default
    short = synth.make_reads([("r", 29_903)], 2000, mixed=True, seed=3)
    assert not M.wants_ops(np.diff(short.cig_off.astype(np.int64)))
    for bam in ("c1.bam", "edge.bam", "mixed.bam"):
        for c in slices(os.path.join(GOLDEN, bam)):
            assert not M.wants_ops(c), bam
    for c in slices(os.path.join(ONT, "ont.bam")):
        assert c.size and M.wants_ops(c)
    assert not M.wants_ops(np.zeros(0, np.uint32))
    # a short-read batch with a minority of complex reads stays
    assert not M.wants_ops(np.concatenate([np.full(900, 3), np.full(100, 400)]))


def test_wants_ops_switch(monkeypatch):
    ont = slices(os.path.join(ONT, "ont.bam"))[0]
    plain = np.ones(100, np.uint32)
    monkeypatch.setenv("BASECOUNT_LONG_READS", "0")
    assert not M.wants_ops(ont) and not M.wants_ops(plain)
    monkeypatch.setenv("BASECOUNT_LONG_READS", "1")
    assert M.wants_ops(ont) and M.wants_ops(plain)
    monkeypatch.delenv("BASECOUNT_LONG_READS")
    assert M.wants_ops(ont) == M.OPS_RULE_DEFAULT and not M.wants_ops(plain)


def test_plan_has_ops_key():
    assert M.PLAN["ops"] == [] or isinstance(M.PLAN["ops"], list)
    assert {"groups", "single", "ops"} <= set(M.PLAN)


def test_ont_goldens_consistent():
    with open(os.path.join(ONT, "manifest.json")) as fh:
        man = json.load(fh)
    assert set(man) == {"ont_default", "ont_shown_long", "ont_q20_m30", "ont_summary", "ont_bed_dp16"}
    for name, c in man.items():
        assert c["bam"] == "ont.bam" and c["returncode"] == 0
        with open(os.path.join(ONT, c["stdout"]), "rb") as fh:
            out = gzip.decompress(fh.read())
        assert hashlib.sha256(out).hexdigest() == c["sha256"], name
        assert os.path.getsize(os.path.join(ONT, c["stdout"])) < (1 << 20)
    assert os.path.getsize(os.path.join(ONT, "ont.bam")) < 110_000
    with BamFile(os.path.join(ONT, "ont.bam")) as f:
        assert f.references == ("ontA", "ontB") and all(2500 <= x <= 3500 for x in f.lengths)
        n_ops = np.diff(f.cig_off.astype(np.int64))
        assert 100 <= f.n_records <= 400
        assert n_ops.min() > 8 and (n_ops > 64).sum() > 10 and (n_ops > 128).sum() > 3
    # the summary case names both references with their read counts
    with open(os.path.join(ONT, man["ont_summary"]["stdout"]), "rb") as fh:
        txt = gzip.decompress(fh.read()).decode()
    assert "ontA" in txt and "ontB" in txt
    bed = open(os.path.join(ONT, "ont.bed")).read().splitlines()
    assert {ln.split("\t")[0] for ln in bed} == {"ontA", "ontB"}
