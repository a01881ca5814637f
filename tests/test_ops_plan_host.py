"""(CPU) bc_ops_plan, k_ops' launch plan (basecount_amd/csrc/bc_ops_plan.h; DESIGN.md §3 "k_ops"):
short-read and unsorted batches get the single window's launch, restated here from DESIGN's
formula; reads longer than half a window get window passes; forced values and their caps hold.
The call reads the batch's header only and needs no device."""
import ctypes as C
import itertools

import pytest

from basecount_amd import device as D

W = 4096


def single_window_rpb(n, L, max_end, seq_bytes, max_span, is_sorted):
    """DESIGN's rule: n/2048 clamped to [32, 8192], and for a sorted batch at most
    (4096 - min(2 seq_bytes / n, max_span, 2048)) x n / max(L, max_end) x 0.75, at least 16."""
    target = min(max(n // 2048, 32), 8192)
    if not is_sorted or L <= 0:
        return target
    density = n / max(L, max_end)
    length = 2.0 * seq_bytes / n if n else 0.0
    if max_span > 0:
        length = min(length, float(max_span))
    fit = (W - min(length, W / 2)) * density * 0.75
    if fit < target:
        target = 16 if fit < 16.0 else int(fit)
    return target


def hdr(n, typical, max_span, max_end, is_sorted=1):
    return dict(n_reads=n, sorted=is_sorted, max_span=max_span, max_end=max_end, seq_bytes=int(n * typical) // 2)


# name -> (header, L): the measured short-read batches of scripts/long_reads.py, the ONT goldens'
# shapes (a few hundred reads of ~600 bp on 3-5 kb), and corners of the rule
SHORT = {
    "artic": (hdr(100_000, 500, 905, 30_000), 30_000),
    "mid1200": (hdr(50_000, 1200, 2100, 30_000), 30_000),
    "ontA": (hdr(240, 610, 1490, 4990), 5000),
    "ontB": (hdr(160, 580, 1310, 3000), 3000),
    "one_read": (hdr(1, 700, 700, 800), 1000),
    "exactly_half_a_window": (hdr(9000, 2048, 3000, 400_000), 400_000),
    "long_but_max_span_short": (hdr(9000, 9000, 2048, 400_000), 400_000),
    "deep": (hdr(40_000_000, 150, 151, 30_000), 30_000),
    "past_the_reference": (hdr(5000, 400, 900, 90_000), 60_000),
}
for _ops in (3, 9, 17, 33, 65, 129):
    SHORT[f"ops{_ops}"] = (hdr(50_000, 500, 700 + _ops, 30_000), 30_000)
LONG = {
    "deep_long": (hdr(40_000, 9000, 9000, 9102), 9102),
    "long": (hdr(20_000, 8000, 14_000, 5_000_000), 5_000_000),
    "long30k": (hdr(5000, 30_000, 52_000, 5_000_000), 5_000_000),
    "just_over_half": (hdr(9000, 2050, 3000, 400_000), 400_000),
    "no_max_span": (hdr(9000, 9000, 0, 400_000), 400_000),
}


def formula(h, L):
    return single_window_rpb(h["n_reads"], L, h["max_end"], h["seq_bytes"], h["max_span"], h["sorted"])


@pytest.mark.parametrize("name", sorted(SHORT))
def test_short_reads_get_the_single_window(name):
    h, L = SHORT[name]
    p = D.ops_plan(h, L)
    rpb = formula(h, L)
    assert p == {"reads_per_block": rpb, "window": W, "passes_max": 1, "blocks": -(-h["n_reads"] // rpb)}, name
    assert D.ops_plan(h, L, 0, 1) == p


@pytest.mark.parametrize("name", sorted(dict(SHORT, **LONG)))
def test_unsorted_batches_have_no_window_and_one_pass(name):
    h, L = dict(SHORT, **LONG)[name]
    u = dict(h, sorted=0)
    for passes in (0, 1, 4, D.OPS_PASSES_MAX):
        p = D.ops_plan(u, L, 0, passes)
        assert p["window"] == 0 and p["passes_max"] == 1 and p["reads_per_block"] == formula(u, L), (name, passes)
        assert p["reads_per_block"] == min(max(h["n_reads"] // 2048, 32), 8192)


def test_the_formula_on_a_grid():
    for n, typical, L, srt in itertools.product((1, 37, 300, 4097, 50_000, 3_000_000), (36, 150, 500, 1200, 2048),
                                                (1, 700, 30_000, 5_000_000, 3_000_000_000), (0, 1)):
        for max_span, max_end in ((0, L), (typical // 2, L), (3 * typical, L + 5000), (70_000, L // 2)):
            h = hdr(n, typical, max_span, max_end, srt)
            p = D.ops_plan(h, L)
            assert (p["reads_per_block"], p["passes_max"]) == (formula(h, L), 1), (h, L)
            assert p["blocks"] == -(-n // p["reads_per_block"])


@pytest.mark.parametrize("name", sorted(LONG))
def test_longer_reads_get_passes(name):
    h, L = LONG[name]
    p = D.ops_plan(h, L)
    assert p["window"] == W and 1 < p["passes_max"] <= D.OPS_PASSES_MAX, p
    assert p["blocks"] == -(-h["n_reads"] // p["reads_per_block"]) and 1 <= p["reads_per_block"] <= 32768
    # the reads that start within one window: at least a read per wave, at most the device-filling target
    density = h["n_reads"] / max(L, h["max_end"])
    assert p["reads_per_block"] == max(4, min(int(W * density), min(max(h["n_reads"] // 2048, 32), 8192))), p
    # what the workgroup's reads can reach, when the batch bounds its spans
    if h["max_span"]:
        starts = p["reads_per_block"] * max(L, h["max_end"]) / h["n_reads"]
        assert p["passes_max"] == min(D.OPS_PASSES_MAX, int((starts + h["max_span"]) / W + 1)), p
    else:
        assert p["passes_max"] == D.OPS_PASSES_MAX
    one = D.ops_plan(h, L, 0, 1)  # passes 1: the single window's own launch
    assert one == {"reads_per_block": formula(h, L), "window": W, "passes_max": 1,
                   "blocks": -(-h["n_reads"] // formula(h, L))}
    for forced in (2, 3, 8, D.OPS_PASSES_MAX):  # forcing the passes leaves the geometry alone
        f = D.ops_plan(h, L, 0, forced)
        assert f == dict(p, passes_max=forced)


def test_forced_values():
    h, L = LONG["long"]
    s, Ls = SHORT["artic"]
    for rpb in (1, 3, 64, 32767, 32768):
        assert D.ops_plan(h, L, rpb)["reads_per_block"] == rpb and D.ops_plan(s, Ls, rpb)["reads_per_block"] == rpb
        assert D.ops_plan(h, L, rpb)["blocks"] == -(-h["n_reads"] // rpb)
        assert D.ops_plan(dict(h, sorted=0), L, rpb)["reads_per_block"] == rpb
    for rpb in (32769, 100_000, 2 ** 31 - 1):  # a 16-bit half counts one workgroup's reads at a position
        assert D.ops_plan(h, L, rpb)["reads_per_block"] == 32768 and D.ops_plan(s, Ls, rpb, 4)["reads_per_block"] == 32768
    for passes in range(2, D.OPS_PASSES_MAX + 1):  # any sorted batch takes forced passes
        assert D.ops_plan(s, Ls, 0, passes) == dict(D.ops_plan(s, Ls), passes_max=passes)
    assert D.ops_plan(h, L, 1)["passes_max"] >= 2  # one read per workgroup still spans windows
    assert D.ops_plan(hdr(0, 0, 0, 0), 1000)["blocks"] == 0


def test_arguments_are_checked():
    L = D.lib()
    assert D.OPS_PASSES_MAX == 16
    r, p = D.BcReads(), D.BcOpsPlan()
    r.n_reads, r.sorted = 10, 1
    assert L.bc_ops_plan(C.byref(r), 100, 0, 0, C.byref(p)) == 0 and p.reserved == 0
    assert L.bc_ops_plan(C.byref(r), 100, 0, D.OPS_PASSES_MAX + 1, C.byref(p)) == D.BC_E_ARG
    assert L.bc_ops_plan(C.byref(r), 100, 0, -1, C.byref(p)) == D.BC_E_ARG
    assert L.bc_ops_plan(C.byref(r), 100, -1, 0, C.byref(p)) == D.BC_E_ARG
    assert L.bc_ops_plan(C.byref(r), -1, 0, 0, C.byref(p)) == D.BC_E_ARG
    assert L.bc_ops_plan(None, 100, 0, 0, C.byref(p)) == D.BC_E_ARG
    assert L.bc_ctx_set_ops_passes(None, 0) == D.BC_E_ARG
    assert L.bc_abi_version() == 8  # symbols were added, nothing changed
