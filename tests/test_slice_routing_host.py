"""Where k_pileup's slice instance is taken (bc_pileup_launch_info; host arithmetic, no GPU needed).
BC_INSTANCE_AUTO takes it where it takes the lean walk (every read one CIGAR op) AND a slice
instance is built (min_base_quality 0, 32-bit indices) AND a read can be longer than a tile
(max_span > 64); BC_INSTANCE_SLICE forces it, and falls back as a forced lean instance does where
none is built.  The library reports it as lean = 1 with BC_SLICE_LDS_BYTES of LDS (the binding's
``slice``).  What tests/test_lean_routing_host.py pins for short reads stays as it is."""
import pytest

from basecount_amd import device as D

L = 29_903


def hdr(n=100_000, words=None, span=150, end=L):
    return {"n_reads": n, "max_span": span, "max_end": end, "n_cigar_words": n if words is None else words}


def kind(info):
    return "slice" if info["slice"] else "lean" if info["lean"] else "general"


def test_c2_shape_takes_slice_at_six_per_cu():
    i = D.pileup_launch_info(hdr(), L)
    assert (i["kernel"], i["lean"], i["slice"], i["waves_per_tile"], i["block_threads"]) == ("tiles", True, True, 4, 256)
    assert i["lds_bytes"] == 4 * (1024 + 4096 + 32) + 1536 + 2048 + 64 == 24_256 == D.slice_lds_bytes(4, 4)
    granules = -(-i["lds_bytes"] // 1280)
    assert granules == 19 and 6 * granules * 1280 == 145_920 <= 160 * 1024 < 7 * granules * 1280
    assert i["blocks"] == D.pileup_plan(hdr(), L)["blocks"]
    # eight-wave blocks: three per CU
    i8 = D.pileup_launch_info(hdr(), L, "tile", 8)
    assert i8["slice"] and i8["lds_bytes"] == 8 * 5152 + 1536 + 2048 + 64 == D.slice_lds_bytes(8, 8)
    assert 3 * -(-i8["lds_bytes"] // 1280) * 1280 <= 160 * 1024 < 4 * -(-i8["lds_bytes"] // 1280) * 1280


def test_auto_rule_span():
    """A read longer than a tile: max_span 65 takes slices, 64 keeps whole reads."""
    assert kind(D.pileup_launch_info(hdr(span=65), L, "tile", 4)) == "slice"
    i = D.pileup_launch_info(hdr(span=64), L, "tile", 4)
    assert kind(i) == "lean" and i["lds_bytes"] == 31_936
    assert kind(D.pileup_launch_info(hdr(span=30), L, "tile", 4)) == "lean"
    assert kind(D.pileup_launch_info(hdr(span=250), L, "tile", 4)) == "slice"


def test_auto_rule_quality_threshold():
    assert kind(D.pileup_launch_info(hdr(), L, "tile", 4, "auto", 0, 5)) == "slice"
    i = D.pileup_launch_info(hdr(), L, "tile", 4, "auto", 20, 5)
    assert kind(i) == "lean" and i["lds_bytes"] == 31_936
    assert kind(D.pileup_launch_info(hdr(), L, "tile", 4, "auto", 0, 6)) == "slice"


def test_auto_rule_one_cigar_word_more_than_reads():
    n = 100_000
    assert kind(D.pileup_launch_info(hdr(n, n), L, "tile", 4)) == "slice"
    g = D.pileup_launch_info(hdr(n, n + 1), L, "tile", 4)
    assert kind(g) == "general" and g["lds_bytes"] == 40_640


def test_forced():
    # forced slice: whatever the spans and the CIGARs
    assert kind(D.pileup_launch_info(hdr(2000, 6000, span=30, end=640), 640, "tile", 4, "slice")) == "slice"
    # a quality threshold (32-bit indices): a forced lean instance
    i = D.pileup_launch_info(hdr(), L, "tile", 4, "slice", 20, 5)
    assert kind(i) == "lean" and i["lds_bytes"] == 31_936
    # 64-bit indices: lean without a threshold, general with one (as BC_INSTANCE_LEAN there)
    big = {"n_reads": 2**31, "max_span": 150, "max_end": 2**33, "n_cigar_words": 2**31}
    assert kind(D.pileup_launch_info(big, 2**33, "tile", 4, "slice", 0, 5)) == "lean"
    assert kind(D.pileup_launch_info(big, 2**33, "tile", 4, "slice", 20, 5)) == "general"
    assert kind(D.pileup_launch_info(big, 2**33, "tile", 4, "auto", 0, 5)) == "lean"
    # forced lean and general stay what they were, long reads or not
    i = D.pileup_launch_info(hdr(), L, "tile", 4, "lean")
    assert kind(i) == "lean" and i["lds_bytes"] == 31_936
    assert kind(D.pileup_launch_info(hdr(), L, "tile", 4, "general")) == "general"


@pytest.mark.parametrize("waves,shape", [(1, "tile_no_solo"), (2, "tile_no_solo"), (4, "tile"), (8, "tile")])
def test_lds_of_every_group_size(waves, shape):
    i = D.pileup_launch_info(hdr(), L, shape, waves, "slice")
    nw = max(4, waves)
    assert i["slice"] and i["waves_per_tile"] == waves and i["block_threads"] == 64 * nw
    assert i["lds_bytes"] == nw * (1024 + 4096 + 32) + (nw // waves) * 1536 + 2048 + 64
    l = D.pileup_launch_info(hdr(), L, shape, waves, "lean")
    assert not l["slice"] and l["lean"] and l["lds_bytes"] - i["lds_bytes"] == nw * (6016 - 4096)


def test_values():
    assert D.INSTANCES == {"auto": 0, "general": 1, "lean": 2, "slice": 4}
    r, out = D.BcReads(), D.BcLaunchInfo()
    assert D.lib().bc_pileup_launch_info(r, 640, 0, 0, 3, 0, 5, out) == -1  # 3 is no BC_INSTANCE_* value
    assert D.lib().bc_pileup_launch_info(r, 640, 0, 0, 5, 0, 5, out) == -1
    assert D.lib().bc_pileup_launch_info(r, 640, 0, 0, 4, 0, 5, out) == 0
    assert D.lib().bc_ctx_set_instance(None, 4) == -1  # (no context: an argument error, not a crash)


def test_answers_pinned_elsewhere_are_unchanged():
    """tests/test_lean_routing_host.py's short-read headers: whole-read lean, 31,936 B."""
    h = {"n_reads": 2000, "max_span": 30, "max_end": 640, "n_cigar_words": 2000}
    i = D.pileup_launch_info(h, 640)
    assert (i["kernel"], i["lean"], i["slice"], i["lds_bytes"]) == ("tiles", True, False, 31_936)
    p = D.pileup_plan(hdr(), L)  # bc_pileup_plan keeps describing the general instance
    assert (p["kernel"], p["waves_per_tile"], p["block_threads"], p["lds_bytes"]) == ("tiles", 4, 256, 40_640)
