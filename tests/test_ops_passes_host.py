"""(CPU) The inputs of test_gpu_ops_passes.py prove themselves: the restatement of k_ops' window
passes in tests/ops_passes.py (which pass owns which event, where a step is split, how many passes a
workgroup runs) finds in every case the piece the case is named for, and no longer finds it in the
case's perturbed twin.  A change to a generator cannot silently turn a case into one more run of
the single window."""
import numpy as np
import pytest

import ops_passes as OP
import saturation_batches as SB
from ops_passes import BASE, CAP, W


def both(name):
    return OP.case(name)[0], OP.case(name, True)[0]


def test_the_model_on_a_hand_made_read():
    ops = [(SB.M, 100), (SB.I, 5), (SB.DEL, 30)] + [(SB.P, 1)] * 61 + [(SB.M, 70)]
    assert OP.ref_ops(ops) == [(0, SB.M, 0, 100), (2, SB.DEL, 100, 30), (64, SB.M, 130, 70)]
    assert OP.steps(ops) == [(0, 64), (64, 128), (128, 130), (130, 194), (194, 200)]  # 64 ops, then 1
    assert [OP.owner(p, 100, 3) for p in (99, 100, 4195, 4196, 8291, 8292, 10 ** 9)] == [0, 0, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("name", OP.cases())
def test_cases_are_sorted_many_pass_batches(name):
    """Every case starts at BASE, is sorted, and takes the passes and reads per block the GPU test
    forces (the plan's own choice is passes for the cases of long reads only)."""
    from basecount_amd import device as D

    b, L = OP.case(name)
    assert int(b["pos"][0]) == BASE and np.all(np.diff(b["pos"]) >= 0)
    assert L <= 45_000 or name == "outlier"
    plan = D.ops_plan(OP.header(b), L)
    assert plan["window"] == W and (plan["passes_max"] > 1) == (2 * b["seq"].size / b["pos"].size > W / 2), plan
    for rpb in OP.RPBS:
        for passes in OP.FORCED:
            p = D.ops_plan(OP.header(b), L, rpb, passes)
            assert (p["reads_per_block"], p["passes_max"]) == (rpb, passes)


@pytest.mark.parametrize("span", OP.SPANS)
def test_span_cases(span):
    b, pb = both(f"span{span}")
    last = (span - 1) // W
    for rpb in OP.RPBS:
        assert OP.read_passes(b, rpb, CAP, 0) == set(range(last + 1))
        assert OP.passes_run(b, rpb, CAP) == [last + 1]
        assert OP.passes_run(b, rpb, 2) == [min(2, last + 1)]
    # the edge itself: the read's last event is a window's last, first, or second position
    assert (span - 1) % W in (W - 2, W - 1, 0)
    assert (SB.spans(pb)[0] - 1) % W not in (W - 2, W - 1, 0)


def test_straddle_case():
    b, pb = both("straddle")
    assert b["pos"].size == 65
    for i in range(1, 64):  # the first workgroup of 64: the anchor and the reads 63 .. 1 before the end
        s = 64 - i
        assert int(b["pos"][i]) == BASE + W - s
        assert s in OP.split_lanes(b, 64, CAP, i) and s in OP.split_lanes(b, 64, 2, i)
        assert OP.read_passes(b, 64, CAP, i) == {0, 1}
        assert not OP.split_lanes(pb, 64, CAP, i)
    assert {64 - i for i in range(1, 64)} == set(range(1, 64))
    assert int(b["pos"][64]) == BASE + W
    assert OP.read_passes(b, 64, CAP, 0) == {0, 1, 2, 3}


def test_across_case():
    b, pb = both("across")
    for rpb in OP.RPBS:  # (every read starts at BASE: every workgroup's window starts there)
        assert SB.DEL in OP.ops_across(b, rpb, CAP, 0) and SB.SKIP in OP.ops_across(b, rpb, CAP, 1)
        assert SB.X in OP.ops_across(b, rpb, CAP, 2) and SB.M in OP.ops_across(b, rpb, CAP, 2)
        assert OP.ops_at_window_end(b, rpb, 3) == [1]                   # the I
        assert OP.ops_at_window_end(b, rpb, 4) == [2, 3, 4, 5, 6, 7]    # 0D 0I 2P 0N 1H 0M
        assert OP.ops_at_window_end(b, rpb, 5) == [3, 6]                # an I at W + 1 - 1 ... and at 2W
    assert SB.DEL not in OP.ops_across(pb, 64, CAP, 0) and SB.SKIP not in OP.ops_across(pb, 64, CAP, 1)
    assert SB.X not in OP.ops_across(pb, 64, CAP, 2)
    assert all(not OP.ops_at_window_end(pb, 64, i) for i in (3, 4, 5))


def test_batch64_case():
    b, pb = both("batch64")
    assert min(b["cig_n"]) > 64
    assert OP.op_batch_starts(b, 64, 0)[0] == W and OP.op_batch_starts(b, 64, 1)[0] == 2 * W
    assert all(x % W for i in (0, 1) for x in OP.op_batch_starts(pb, 64, i))


def test_late_and_gap_cases():
    b, pb = both("late")
    for i in range(1, b["pos"].size):
        assert BASE + 3000 <= int(b["pos"][i]) < BASE + W
        assert {0, 1, 2, 3} <= OP.read_passes(b, 64, CAP, i)
        assert max(OP.read_passes(pb, 64, CAP, i)) == 1
    b, pb = both("gap")
    owned = [OP.read_passes(b, 64, CAP, i) for i in range(4)]
    assert owned[0] == owned[1] == {0} and min(owned[2]) == 2 and 1 not in set().union(*owned)
    assert OP.passes_run(b, 64, CAP) == [4] and OP.passes_run(b, 64, 3) == [3]
    assert OP.passes_run(pb, 64, CAP) == [2]


def test_early_case():
    b, pb = both("early")
    assert OP.passes_run(b, 64, 8) == [2] and OP.passes_run(b, 64, CAP) == [2]
    assert OP.passes_run(pb, 64, 8) == [4]


def test_outlier_case():
    b, pb = both("outlier")
    ends = b["pos"].astype(np.int64) + SB.spans(b)
    assert int(np.argmax(ends)) == 7 and (int(ends[7]) - 1 - BASE) // W >= CAP  # beyond the last pass's window
    assert SB.SKIP in OP.ops_across(b, 64, CAP, 7) and OP.passes_run(b, 64, CAP) == [CAP]
    assert sorted(ends)[-2] - BASE < 3 * W
    assert (int((pb["pos"].astype(np.int64) + SB.spans(pb)).max()) - BASE) // W < CAP


def test_cut_case():
    (b, L), (pb, pL) = OP.case("cut"), OP.case("cut", True)
    assert BASE + 2 * W < L < BASE + 3 * W
    ends = b["pos"].astype(np.int64) + SB.spans(b)
    assert list(np.flatnonzero(ends > L)) == [6, 12, 13]
    assert SB.expect(b, L, 0)[1] == 6 and SB.expect(pb, pL, 0)[1] == -1
    assert OP.block_of(b, 3, 6)[0] != OP.block_of(b, 3, 12)[0]  # bad reads in two workgroups of 3
    assert min(OP.read_passes(b, 64, CAP, 13)) == 3 and OP.read_passes(b, 64, CAP, 12) == {2}
    # read 6 has a step split at the end of pass 2, all of whose events lie at or beyond L
    p0 = int(b["pos"][6])
    split = [(e0, e1) for e0, e1 in OP.steps(OP.cigars(b)[6])
             if OP.owner(p0 + e0, BASE, CAP) == 2 and OP.owner(p0 + e1 - 1, BASE, CAP) == 3]
    assert split and all(p0 + e0 >= L for e0, _ in split)


def test_nbases_case():
    b, pb = both("nbases")
    nib = np.stack([b["seq"] >> 4, b["seq"] & 15], 1).ravel()
    for i, letter in enumerate((SB.N, SB.EQ, SB.N)):
        at = int(b["seq_nib"][i])
        for edge in (W, 2 * W):
            assert set(nib[at + edge - 2: at + edge + 2]) == {letter}
    assert {19, 20} == set(b["qual"][: 3 * W])
    pn = np.stack([pb["seq"] >> 4, pb["seq"] & 15], 1).ravel()
    assert len(set(pn[W - 2: W + 2]) | set(pn[2 * W - 2: 2 * W + 2])) > 1


def test_deep_batches():
    for d in (300, 40_000):
        b, one, L = OP.deep_batch(d)
        assert b["pos"].size == d and set(b["pos"]) == {BASE} and L > BASE + 2 * W
        assert int(one["cig_n"][0]) > 64 and OP.read_passes(one, 1, CAP, 0) == {0, 1, 2}
    assert 40_000 > 32768  # more than one workgroup may take: the run is cut
