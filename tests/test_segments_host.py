"""Grouped references, host side (no GPU): the virtual-reference layout (bc_segments_layout
through ctypes) and the pure planner that decides which references of a batch share a launch."""
import ctypes as C

import numpy as np
import pytest

from basecount_amd import device as D
from basecount_amd import main as M


def _layout_rc(lens):
    a = np.ascontiguousarray(lens, np.int64)
    out = np.full(a.size + 1, -7, np.int64)
    rc = D.lib().bc_segments_layout(a.ctypes.data if a.size else None, int(a.size), out.ctypes.data)
    return rc, out


def test_segments_layout_offsets_are_64_aligned_prefix_sums():
    rc, voff = _layout_rc([1, 63, 64, 65, 8193])
    assert rc == 0
    assert voff.tolist() == [0, 64, 128, 192, 320, 8576]
    assert D.segments_layout([1, 63, 64, 65, 8193]).tolist() == [0, 64, 128, 192, 320, 8576]
    assert D.segments_layout([5]).tolist() == [0, 64]


@pytest.mark.parametrize("lens", [[10, 0, 10], [10, -3], [0], [-1]])
def test_segments_layout_rejects_empty_and_negative_lengths(lens):
    rc, _ = _layout_rc(lens)
    assert rc == D.BC_E_ARG
    assert b"length" in D.lib().bc_last_error()
    with pytest.raises(D.BcError) as ei:
        D.segments_layout(lens)
    assert ei.value.code == D.BC_E_ARG


def test_segments_layout_rejects_no_segments():
    a = np.ones(1, np.int64)
    out = np.zeros(2, np.int64)
    assert D.lib().bc_segments_layout(a.ctypes.data, 0, out.ctypes.data) == D.BC_E_ARG
    assert D.lib().bc_segments_layout(a.ctypes.data, -1, out.ctypes.data) == D.BC_E_ARG
    assert D.lib().bc_segments_layout(None, 1, out.ctypes.data) == D.BC_E_ARG
    with pytest.raises(D.BcError):
        D.segments_layout([])


def test_segments_layout_int32_limit():
    """Starts are int32: the virtual reference may span at most 2^31 - 128 positions."""
    top = 2**31 - 128
    assert D.segments_layout([top]).tolist() == [0, top]
    assert D.segments_layout([top - 64, 64]).tolist() == [0, top - 64, top]
    assert D.segments_layout([top - 64, 1]).tolist() == [0, top - 64, top]  # the pad counts
    for lens in ([top + 1], [top - 64, 65], [2**30, 2**30, 64], [2**62, 2**62], [2**63 - 1, 2**63 - 1]):
        rc, _ = _layout_rc(lens)
        assert rc == D.BC_E_ARG, lens
        assert b"2^31" in D.lib().bc_last_error()


def test_pileup_segments_checks_arguments_before_any_device():
    L = D.lib()
    args = (None, None, None, 64, None, 0, 5, 0.0, 0.0, None, None, None, None, None, None)
    assert L.bc_pileup_segments(None, None, 1, *args) == D.BC_E_ARG
    assert b"NULL" in L.bc_last_error()
    assert hasattr(L, "bc_segments_layout") and isinstance(L.bc_segments_layout, C._CFuncPtr)


# ---- the planner ---------------------------------------------------------------------------------
def test_plan_groups_all_eligible_under_cap_is_one_group():
    lens = [1000, 2000, 64, 1, 5000]
    assert M.plan_groups(lens, [True] * 5, 1 << 24) == [[0, 1, 2, 3, 4]]


def test_plan_groups_ineligible_reference_splits_a_run():
    lens = [100] * 7
    elig = [True, True, True, False, True, True, True]
    assert M.plan_groups(lens, elig, 1 << 24) == [[0, 1, 2], [4, 5, 6]]


def test_plan_groups_single_reference_runs_are_dropped():
    lens = [100] * 8
    elig = [True, False, True, True, False, False, True, False]
    assert M.plan_groups(lens, elig, 1 << 24) == [[2, 3]]
    assert M.plan_groups([100], [True], 1 << 24) == []
    assert M.plan_groups([], [], 1 << 24) == []
    assert M.plan_groups(lens, [False] * 8, 1 << 24) == []


def test_plan_groups_cap_cuts_a_run_on_padded_lengths():
    # every length occupies round_up(L, 64) virtual positions: 65 -> 128
    lens = [65, 65, 65, 65, 65]
    assert M.plan_groups(lens, [True] * 5, 256) == [[0, 1], [2, 3]]  # the last run is one reference
    assert M.plan_groups(lens, [True] * 5, 384) == [[0, 1, 2], [3, 4]]
    assert M.plan_groups(lens, [True] * 5, 640) == [[0, 1, 2, 3, 4]]
    assert M.plan_groups(lens, [True] * 5, 639) == [[0, 1, 2, 3]]
    for g in M.plan_groups([1000, 3000, 200, 64, 4000, 100, 100], [True] * 7, 4096):
        assert sum((L + 63) // 64 * 64 for L in ([1000, 3000, 200, 64, 4000, 100, 100][t] for t in g)) <= 4096


def test_plan_groups_reference_longer_than_cap_stays_alone():
    lens = [100, 100, 5000, 100, 100]
    assert M.plan_groups(lens, [True] * 5, 1024) == [[0, 1], [3, 4]]


def test_plan_groups_first_offsets_the_refids():
    assert M.plan_groups([10, 10, 10], [True, True, True], 1 << 20, first=40) == [[40, 41, 42]]


def test_plan_groups_follows_refid_order_only():
    """Grouping is a function of lengths and eligibility by refID: numpy inputs give the same."""
    lens = np.array([300, 200, 100, 50], np.int64)
    elig = np.array([True, True, False, True])
    assert M.plan_groups(lens, elig, 1 << 24) == [[0, 1]]
    assert all(isinstance(t, int) for g in M.plan_groups(lens, elig, 1 << 24) for t in g)


def test_reads_inside_flags_unsorted_overhanging_and_negative():
    #            ref0: fine   ref1: unsorted   ref2: overhang   ref3: none   ref4: negative start
    ref_beg = np.array([0, 2, 4, 5, 5, 6], np.int64)
    pos = np.array([0, 90, 50, 10, 95, -1], np.int32)
    span = np.array([10, 10, 10, 10, 10, 5], np.int64)
    lens = np.array([100, 100, 104, 30, 100], np.int64)
    assert M._reads_inside(pos, span, ref_beg, lens).tolist() == [True, False, False, True, False]
    # a start that drops at a reference boundary is not "unsorted"; ending exactly at L is inside
    ref_beg = np.array([0, 1, 2], np.int64)
    ok = M._reads_inside(np.array([90, 0], np.int32), np.array([10, 100], np.int64), ref_beg,
                         np.array([100, 100], np.int64))
    assert ok.tolist() == [True, True]


def test_group_cap_environment(monkeypatch):
    monkeypatch.delenv("BASECOUNT_GROUP_REFS", raising=False)
    monkeypatch.delenv("BASECOUNT_GROUP_MAX", raising=False)
    assert M.group_cap() == 1 << 24
    monkeypatch.setenv("BASECOUNT_GROUP_MAX", "4096")
    assert M.group_cap() == 4096
    monkeypatch.setenv("BASECOUNT_GROUP_REFS", "0")
    assert M.group_cap() == 0
