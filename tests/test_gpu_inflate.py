"""k_inflate through bc_bgzf_inflate against zlib: the vectors of tests/inflate_vectors.py packed back
to back (unaligned coff / uoff), sentinel guards around input and output and between the blocks.
The invalid list is a bounds check of a correct kernel under the contract's equivalence "status 0
exactly where zlib accepts, and then the same bytes"; the host sanitizer program (tests/test_inflate_host.py) runs the same header
on the same vectors."""
import numpy as np
import pytest

import inflate_vectors as V
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

GUARD = 509  # odd: the first block starts unaligned
IN_SENT, OUT_SENT = 0xC3, 0x9E


@pytest.fixture(scope="module")
def ctx():
    c = D.Context(0)
    yield c
    c.close()


def pack(vecs):
    """(comp bytes, out template, descriptors): blocks back to back, 0..3 sentinel bytes between
    the outputs of neighbours."""
    blocks = np.zeros(len(vecs), D.ZBLOCK_DTYPE)
    coff, uoff = GUARD, GUARD
    for i, x in enumerate(vecs):
        blocks[i] = (coff, len(x.comp), x.isize, uoff)
        coff += len(x.comp)
        uoff += x.isize + i % 4
    comp = np.full(coff + GUARD, IN_SENT, np.uint8)
    for b, x in zip(blocks, vecs):
        comp[int(b["coff"]):int(b["coff"]) + len(x.comp)] = np.frombuffer(x.comp, np.uint8)
    return comp, np.full(uoff + GUARD, OUT_SENT, np.uint8), blocks


def inflate(ctx, comp, out0, blocks, calls):
    """Run `calls` (slices of the block list, one bc_bgzf_inflate each); returns (out, status)."""
    d_comp = ctx.alloc(comp.size).upload(comp)
    d_out = ctx.alloc(out0.size).upload(out0)
    d_blocks = ctx.alloc(blocks.nbytes).upload(blocks)
    d_status = ctx.alloc(len(blocks)).upload(np.full(len(blocks), 0xFF, np.uint8))
    for lo, hi in calls:
        ctx.bgzf_inflate(d_comp.ptr, comp.size, d_blocks.ptr + 24 * lo, hi - lo, d_out.ptr, out0.size,
                         d_status.ptr + lo)
    out = d_out.download(np.uint8, out0.size)
    status = d_status.download(np.uint8, len(blocks))
    assert np.array_equal(d_comp.download(np.uint8, comp.size), comp)  # the input is read-only
    for b in (d_comp, d_out, d_blocks, d_status):
        b.free()
    return out, status


def check(vecs, blocks, out, status, must_accept):
    covered = np.zeros(out.size, bool)
    for x, b, st in zip(vecs, blocks, status):
        lo = int(b["uoff"])
        got = out[lo:lo + x.isize].tobytes()
        covered[lo:lo + x.isize] = True
        if must_accept:
            assert st == 0, "%s: status %d" % (x.name, st)
            assert got == x.expect, x.name
        else:
            V.check_rule(x, int(st), got)
    # guards and every byte between the blocks are as they were
    assert np.all(out[~covered] == OUT_SENT)


def test_valid_vectors_in_one_call(ctx):
    comp, out0, blocks = pack(V.VALID)
    out, status = inflate(ctx, comp, out0, blocks, [(0, len(blocks))])
    check(V.VALID, blocks, out, status, True)


def test_valid_vectors_one_call_per_block(ctx):
    comp, out0, blocks = pack(V.VALID)
    out, status = inflate(ctx, comp, out0, blocks, [(i, i + 1) for i in range(len(blocks))])
    check(V.VALID, blocks, out, status, True)


def test_thousand_blocks_in_one_call(ctx):
    """The vectors cycled: a wave's tables and buffers left over from its previous block show."""
    small = [x for x in V.VALID if x.isize < 65535] + [x for x in V.VALID if x.isize >= 65535][:4]
    vecs = [small[i % len(small)] for i in range(1000)]
    comp, out0, blocks = pack(vecs)
    out, status = inflate(ctx, comp, out0, blocks, [(0, 1000)])
    check(vecs, blocks, out, status, True)


def test_invalid_vectors_obey_the_rule(ctx):
    comp, out0, blocks = pack(V.INVALID)
    out, status = inflate(ctx, comp, out0, blocks, [(0, len(blocks))])
    check(V.INVALID, blocks, out, status, False)
    assert np.count_nonzero(status) > len(V.INVALID) // 2
    by = dict(zip((x.name for x in V.INVALID), status))
    for name in V.NAMED_INVALID:
        assert by[name] != 0, name


def test_descriptors_outside_their_buffers_are_refused(ctx):
    """The kernel checks each descriptor itself: a failing block is skipped with status 1."""
    x = V.VALID[1]
    comp, out0, blocks = pack([x] * 5)
    blocks[1]["coff"] = comp.size - 3  # coff + clen past comp_bytes
    blocks[2]["uoff"] = out0.size - x.isize + 1  # uoff + isize past out_bytes
    blocks[3]["isize"] = 65537
    out, status = inflate(ctx, comp, out0, blocks, [(0, 5)])
    assert list(status) == [0, 1, 1, 1, 0]
    for i in (0, 4):
        lo = int(blocks[i]["uoff"])
        assert out[lo:lo + x.isize].tobytes() == x.expect
    keep = np.ones(out.size, bool)
    for i in (0, 4):
        keep[int(blocks[i]["uoff"]):int(blocks[i]["uoff"]) + x.isize] = False
    assert np.all(out[keep] == OUT_SENT)


def test_host_entry_point_matches(ctx):
    """bc_bgzf_inflate_host: upload, kernel, download; bytes of the output outside the blocks stay."""
    comp, out0, blocks = pack(V.VALID)
    out = out0.copy()
    status = ctx.bgzf_inflate_host(comp, blocks, out)
    check(V.VALID, blocks, out, status, True)
    t = ctx.bgzf_inflate_times()
    assert t["blocks"] >= len(blocks) and t["kernel_ms"] > 0


def test_host_entry_point_inflates_the_fuzz_streams(ctx):
    """The structured fuzz streams (random code sets, headers and block mixes) once more, through
    bc_bgzf_inflate_host and in reverse order: other neighbours, other alignments."""
    by = {x.name: x for x in V.VALID}
    vecs = [by[name] for name in reversed(V.FUZZ_NAMES)]
    assert len(vecs) >= 300
    comp, out0, blocks = pack(vecs)
    out = out0.copy()
    status = ctx.bgzf_inflate_host(comp, blocks, out)
    check(vecs, blocks, out, status, True)


def test_host_entry_point_refuses_bad_descriptors(ctx):
    x = V.VALID[1]
    comp, out0, blocks = pack([x] * 4)
    blocks[1]["isize"] = 1 << 30
    blocks[2]["coff"] = comp.size
    out = out0.copy()
    status = ctx.bgzf_inflate_host(comp, blocks, out)
    assert list(status) == [0, 1, 1, 0]
    keep = np.ones(out.size, bool)
    for i in (0, 3):
        lo = int(blocks[i]["uoff"])
        assert out[lo:lo + x.isize].tobytes() == x.expect
        keep[lo:lo + x.isize] = False
    assert np.all(out[keep] == OUT_SENT)


def test_null_and_negative_arguments_are_rejected():
    L = D.lib()
    assert L.bc_bgzf_inflate(None, None, 0, None, 0, None, 0, None) == D.BC_E_ARG
    assert L.bc_bgzf_inflate_host(None, None, 0, None, 0, None, 0, None) == D.BC_E_ARG
