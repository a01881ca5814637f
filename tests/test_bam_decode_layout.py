"""The synthetic inputs of the BAM record decode tests hold the pieces they are meant to hold, proved
from the builder's record offsets alone (tests/bam_decode_inputs.py): no decoder runs here."""
import pytest

import bam_decode_inputs as B

SEGS = (256, 1024, B.DEFAULT_SEG)


@pytest.fixture(scope="module")
def layout():
    b = B.layout_builder()
    return b, b.starts, b.ends, b.size


@pytest.mark.parametrize("seg", SEGS)
def test_layout_pieces_at_each_segment_size(layout, seg):
    b, starts, ends, size = layout
    assert any(s % seg == 0 for s in starts), "a record start exactly on a segment boundary"
    for k in (1, 2, 3):  # the length prefix straddles the boundary
        assert any(s % seg == seg - k for s in starts), "a start in the last %d byte(s) of a segment" % k
    nseg = (size + seg - 1) // seg
    assert set(range(nseg)) - {s // seg for s in starts}, "segments with no start"
    assert any((e - 1) // seg - s // seg >= 2 for s, e in zip(starts, ends)), "a record spanning three segments"


def test_layout_has_one_read_longer_than_a_segment_and_a_bgzf_block(layout):
    b, starts, ends, size = layout
    long = [i for i, r in enumerate(b.recs) if bytes(r[36:43]) == b"long70k"]
    assert len(long) == 1
    r = b.recs[long[0]]
    l_seq = int.from_bytes(r[20:24], "little")
    fields = 36 + 8 + 4 * int.from_bytes(r[16:18], "little") + (l_seq + 1) // 2 + l_seq
    assert 65536 < 68_000 < fields < 72_000  # about 70 kb of fields, before any padding
    assert ends[long[0]] - starts[long[0]] > B.DEFAULT_SEG


def test_layout_ends_exactly_at_the_buffer_end_and_can_be_cut_into_a_partial_record(layout):
    b, starts, ends, size = layout
    assert ends[-1] == size == len(b.raw())
    assert starts == sorted(starts) and all(e == s for e, s in zip(ends, starts[1:]))
    assert starts[0] == b.first == B.header_info(b.raw())[0]
    assert ends[-1] - starts[-1] > 5  # the tests drop 5 bytes: the last record becomes partial


def test_trap_field_is_tiled_by_records_and_reaches_into_the_next_records_segment():
    b, t = B.trap_builder()
    starts, ends = b.starts, b.ends
    r = bytes(b.recs[t])
    l_seq = int.from_bytes(r[20:24], "little")
    n_cigar = int.from_bytes(r[16:18], "little")
    qual_beg = starts[t] + 36 + r[12] + 4 * n_cigar + (l_seq + 1) // 2
    qual_end = qual_beg + l_seq
    assert qual_end == ends[t] == starts[t + 1]  # the field ends the record: no auxiliary bytes
    # the field is a chain of serialized records that ends exactly at its end
    fake, q = [], qual_beg
    raw = b.raw()
    while q < qual_end:
        fake.append(q)
        q += 4 + int.from_bytes(raw[q:q + 4], "little")
    assert q == qual_end and len(fake) >= 10
    genuine = {bytes(x) for x in b.recs[:t]}
    assert all(raw[a:z] in genuine for a, z in zip(fake, fake[1:] + [qual_end]))
    seg = 1024
    assert qual_end // seg - qual_beg // seg >= 3, "the field crosses several segment boundaries"
    last = starts[t + 1] // seg
    assert starts[t + 1] % seg != 0 and last * seg > qual_beg  # that segment starts inside the field
    # a copied record starts in that segment before the true one: the speculation has something to believe
    assert any(last * seg <= f < starts[t + 1] for f in fake)
    # segments wholly inside the trap record hold copied starts and no true one
    inside = [s for s in range(starts[t] // seg + 1, last) if any(s * seg <= f < (s + 1) * seg for f in fake)]
    assert len(inside) >= 2 and not any(st // seg in inside for st in starts)
