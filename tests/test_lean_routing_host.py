"""Which k_pileup instance a batch takes (bc_pileup_launch_info; host arithmetic, no GPU needed):
the lean instance while (n_cigar_words - n_reads) / 2, the bound on multi-run reads, is zero (the
measured fraction), the general one above; forced instances; a slice that shares a larger batch's
CIGAR buffer; and bc_pileup_plan's unchanged answers (it keeps describing the general instance)."""
import pytest

from basecount_amd import device as D

L = 640


def hdr(n, words=None, span=30):
    return {"n_reads": n, "max_span": span, "max_end": L, "n_cigar_words": n if words is None else words}


def test_all_m_batch_takes_lean():
    i = D.pileup_launch_info(hdr(2000), L)
    assert (i["kernel"], i["lean"], i["waves_per_tile"], i["block_threads"]) == ("tiles", True, 4, 256)
    assert i["lds_bytes"] == 4 * (1024 + 6016 + 32) + 1536 + 2048 + 64 == 31_936
    assert 5 * -(-i["lds_bytes"] // 1280) * 1280 <= 160 * 1024  # five workgroups after granule rounding
    assert i["blocks"] == D.pileup_plan(hdr(2000), L)["blocks"]


@pytest.mark.parametrize("n", [2000, 2001, 16_000])
def test_fraction_threshold(n):
    """slow <= (words - n) / 2, and the measured fraction is zero (the lean instance is behind from
    one slow read in 64 on): lean only when every read has one op, general above."""
    assert D.pileup_launch_info(hdr(n, n), L, "tile", 4)["lean"]
    assert not D.pileup_launch_info(hdr(n, n + 1), L, "tile", 4)["lean"]  # (bound 1/2: not provably none)
    assert not D.pileup_launch_info(hdr(n, n + 2), L, "tile", 4)["lean"]  # one read with three ops
    assert not D.pileup_launch_info(hdr(n, n + 2 * (n // 64)), L, "tile", 4)["lean"]  # 1/64 of the reads
    assert not D.pileup_launch_info(hdr(n, 3 * n), L, "tile", 4)["lean"]  # an indel in every read


def test_forced_instances_and_tile_waves():
    for waves in (2, 4, 8):
        shape = "tile_no_solo" if waves == 2 else "tile"
        g = D.pileup_launch_info(hdr(2000), L, shape, waves, "general")
        l = D.pileup_launch_info(hdr(2000, 6000), L, shape, waves, "lean")
        assert (g["lean"], l["lean"]) == (False, True)
        assert g["waves_per_tile"] == l["waves_per_tile"] == waves and g["block_threads"] == l["block_threads"]
        p = D.pileup_plan(hdr(2000), L, shape, waves)
        assert (g["lds_bytes"], g["blocks"], g["block_threads"]) == (p["lds_bytes"], p["blocks"], p["block_threads"])
        assert l["lds_bytes"] < g["lds_bytes"]


def test_where_no_lean_instance_is_built():
    """A quality threshold with 64-bit indices keeps the general instance even when lean is asked for."""
    big = {"n_reads": 2**31, "max_span": 30, "max_end": 2**33, "n_cigar_words": 2**31}
    assert D.pileup_launch_info(big, 2**33, "tile", 4, "lean", 20, 5)["lean"] is False
    assert D.pileup_launch_info(big, 2**33, "tile", 4, "lean", 0, 5)["lean"] is True
    assert D.pileup_launch_info(hdr(2000), L, "tile", 4, "auto", 20, 6)["lean"] is True


def test_other_kernels_report_no_instance():
    assert D.pileup_launch_info(hdr(100), L)["kernel"] == "solo" and not D.pileup_launch_info(hdr(100), L)["lean"]
    i = D.pileup_launch_info(hdr(20_000), L)
    assert i["kernel"] == "rc" and not i["lean"]


def test_slice_is_judged_by_the_buffer_it_shares():
    """Two slices of one upload share its CIGAR buffer and n_cigar_words (the buffer's count): an
    all-M slice beside a slice full of indels is not routed by a count that is neither's own, it
    keeps the general instance; alone (its own buffer) it takes the lean one."""
    n_a, n_b = 2000, 2000
    words_a, words_b = n_a, 3 * n_b
    shared = words_a + words_b
    a = D.BcReads()
    a.n_reads, a.max_span, a.max_end, a.sorted, a.seq_layout = n_a, 30, L, 1, D.BC_SEQ_EVENT
    a.n_cigar_words = shared
    assert not D.pileup_launch_info(a, L, "tile", 4)["lean"]
    a.n_cigar_words = words_a
    assert D.pileup_launch_info(a, L, "tile", 4)["lean"]
    # the bound can only be too large for a slice, never too small: n_cigar_words >= its own words
    assert (shared - n_b) / 2 >= (words_b - n_b) / 2


def test_pileup_plan_unchanged():
    p = D.pileup_plan(hdr(2000), L)
    assert (p["kernel"], p["waves_per_tile"], p["block_threads"], p["lds_bytes"]) == ("tiles", 4, 256, 40_640)
    p8 = D.pileup_plan(hdr(2000), L, "tile", 8)
    assert (p8["block_threads"], p8["lds_bytes"]) == (512, 8 * (3072 + 6176) + 1536 + 2048 + 64)


def test_bad_arguments():
    with pytest.raises(D.BcError):
        D.pileup_launch_info(hdr(10), L, k=7)
    r = D.BcReads()
    out = D.BcLaunchInfo()
    assert D.lib().bc_pileup_launch_info(r, L, 0, 0, 3, 0, 5, out) == -1  # unknown BC_INSTANCE_*
