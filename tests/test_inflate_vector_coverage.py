"""What the VALID list of tests/inflate_vectors.py exercises, found again in the finished streams.

Encoders leave whole parts of bc_inflate.h untouched (zlib run-length-codes the litlen and the
distance lengths apart, always sends two distance codes, never follows a stored block with a match
into it), so the streams that reach those parts are assembled by hand.  This ledger keeps the list
from eroding: a small inflate of its own (nothing shared with the writers of inflate_vectors.py, and
checked against zlib.decompress on every VALID vector) parses each stream and records the features
below, and each must occur."""
import os
import re
import zlib

import pytest

import inflate_vectors as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def len_base_extra(i):  # length symbol 257 + i
    if i < 8:
        return 3 + i, 0
    if i == 28:
        return 258, 0
    e = i // 4 - 1
    return 3 + ((4 + i % 4) << e), e


def dist_base_extra(i):
    if i < 4:
        return 1 + i, 0
    e = i // 2 - 1
    return 1 + ((2 + i % 2) << e), e


def decode_table(lens):
    """(table indexed by the next `width` stream bits -> symbol << 4 | length, width)."""
    width = max(lens) if any(lens) else 0
    table = [0] * (1 << width)
    code = 0
    for n in range(1, width + 1):
        for sym, m in enumerate(lens):
            if m == n:
                rev = int(format(code, "0%db" % n)[::-1], 2)
                table[rev::1 << n] = [sym << 4 | n] * (1 << (width - n))
                code += 1
        code <<= 1
    return table, width


FIXED_LIT = decode_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = decode_table([5] * 32)


def inflate(stream):
    """(output bytes, features of the stream as a set of strings and tuples)."""
    seen = set()
    data = bytes(stream) + bytes(8)
    out, from_stored = bytearray(), bytearray()  # from_stored[i]: out[i] was copied by a stored block
    acc = cnt = p = 0

    def take(n):
        nonlocal acc, cnt, p
        while cnt < n:
            acc |= data[p] << cnt
            p += 1
            cnt += 8
        v = acc & ((1 << n) - 1)
        acc >>= n
        cnt -= n
        return v

    def symbol(tab):
        nonlocal acc, cnt, p
        table, width = tab
        while cnt < width:
            acc |= data[p] << cnt
            p += 1
            cnt += 8
        e = table[acc & ((1 << width) - 1)]
        assert e, "bits that are no code"
        acc >>= e & 15
        cnt -= e & 15
        return e >> 4, e & 15

    while True:
        last, kind = take(1), take(2)
        assert kind != 3
        if kind == 0:
            pad = cnt % 8
            take(pad)
            seen.add(("stored_pad", pad))
            n, inv = take(16), take(16)
            assert n ^ inv == 0xFFFF and cnt % 8 == 0
            p -= cnt // 8
            acc = cnt = 0
            out += data[p:p + n]
            from_stored += b"\1" * n
            p += n
            assert p <= len(stream)
        else:
            if kind == 1:
                lit, dist = FIXED_LIT, FIXED_DIST
            else:
                hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                assert hlit <= 286 and hdist <= 30
                seen.add(("hclen", hclen))
                cl = [0] * 19
                for i in range(hclen):
                    cl[ORDER[i]] = take(3)
                assert sum(1 << (7 - n) for n in cl if n) == 128, "code-length code not complete"
                cltab = decode_table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s, n = symbol(cltab)
                    seen.add(("clen_code_bits", n))
                    if s < 16:
                        lens.append(s)
                        continue
                    rep = 3 + take(2) if s == 16 else 3 + take(3) if s == 17 else 11 + take(7)
                    assert s != 16 or lens
                    if len(lens) < hlit < len(lens) + rep:
                        seen.add(("crossing", s))
                    lens += [lens[-1] if s == 16 else 0] * rep
                assert len(lens) == hlit + hdist and lens[256]
                ll, dl = lens[:hlit], lens[hlit:]
                for name, a in (("litlen", ll), ("dist", dl)):
                    space = sum(1 << (15 - n) for n in a if n)
                    assert space == 32768 or (name == "dist" and space == 0) or (space == 16384 and max(a) == 1)
                ndist = sum(1 for n in dl if n)
                if ndist == 0:
                    seen.add("no_dist_code")
                lit, dist = decode_table(ll), decode_table(dl)
                order = sorted((n, s) for s, n in enumerate(ll) if n)
                late = set(s for n, s in order[256:])  # canonical rank 256 and above
            dyn = kind == 2
            while True:
                s, n = symbol(lit)
                if dyn:
                    seen.add(("litlen_bits", n))
                    if s in late:
                        seen.add(("late_litlen_bits", n))
                if s < 256:
                    out.append(s)
                    from_stored.append(0)
                    continue
                if s == 256:
                    break
                assert s <= 285
                base, extra = len_base_extra(s - 257)
                length = base + take(extra)
                if s == 284 and length == 258:
                    seen.add("258_as_284_31")
                d, dn = symbol(dist)
                assert d <= 29
                base, extra = dist_base_extra(d)
                x = take(extra)
                if dyn:
                    seen.add(("dist_bits", dn))
                    if n == 15 and s == 284 and dn == 15 and extra == 13 and x == 8191:
                        seen.add("15+5_then_15+13_ones")
                    if dn == 15 and extra == 13:
                        seen.add("13_extra_after_15_bits")
                    if ndist == 1:
                        seen.add("one_dist_code_used")
                back = base + x
                assert back <= len(out)
                at = len(out)
                if any(from_stored[at - back:at - back + min(length, back)]):
                    seen.add("match_into_stored")
                if back >= length:
                    out += out[at - back:at - back + length]
                else:
                    for i in range(length):
                        out.append(out[at - back + i])
                from_stored += bytes(length)
        if last:
            break
    assert p - cnt // 8 <= len(stream)
    return bytes(out), seen


@pytest.fixture(scope="module")
def ledger():
    """feature -> the vectors that show it; the parser pinned to zlib on the way."""
    where = {}
    for x in V.VALID:
        out, seen = inflate(x.comp)
        assert out == zlib.decompress(x.comp, -15) == x.expect, x.name
        for f in seen:
            where.setdefault(f, []).append(x.name)
    return where


def roots():
    """BCZ_LIT_ROOT and BCZ_DIST_ROOT as the header sets them."""
    with open(os.path.join(REPO, "basecount_amd", "csrc", "bc_inflate.h")) as f:
        text = f.read()
    return tuple(int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) for name in ("BCZ_LIT_ROOT", "BCZ_DIST_ROOT"))


def test_fifteen_bit_codes_are_used_in_data(ledger):
    assert ("litlen_bits", 15) in ledger and ("dist_bits", 15) in ledger
    assert "13_extra_after_15_bits" in ledger
    # the bit reader's worst case: 15 + 5 bits, then 15 + 13 bits with every extra bit set
    assert "15+5_then_15+13_ones" in ledger


def test_code_lengths_around_the_primary_tables_are_used(ledger):
    lit_root, dist_root = roots()
    assert 1 < lit_root < 15 and 1 < dist_root < 15
    for n in (lit_root, lit_root + 1):
        assert ("litlen_bits", n) in ledger, n
    for n in (dist_root, dist_root + 1):
        assert ("dist_bits", n) in ledger, n


def test_long_codes_beyond_256_shorter_ones_are_used(ledger):
    """A code longer than the primary table's index whose canonical rank is 256 or more."""
    lit_root, _ = roots()
    assert any(("late_litlen_bits", n) in ledger for n in range(lit_root + 1, 16))
    assert "walk_past_256" in ledger[("late_litlen_bits", lit_root + 1)]
    assert "many_15bit" in ledger[("late_litlen_bits", 15)]


def test_repeat_codes_cross_the_litlen_distance_boundary(ledger):
    for s in (16, 17, 18):
        assert ("crossing", s) in ledger, s


def test_distance_sets_of_one_code_and_of_none(ledger):
    assert "one_dist_code_used" in ledger and "no_dist_code" in ledger


def test_code_length_code_extremes(ledger):
    assert ("hclen", 5) in ledger and ("hclen", 19) in ledger
    assert ("hclen", 4) not in ledger  # cannot carry an end-of-block: only INVALID has it
    assert ("clen_code_bits", 7) in ledger


def test_stored_headers_at_every_bit_alignment(ledger):
    for pad in range(8):
        assert ("stored_pad", pad) in ledger, pad


def test_matches_into_stored_bytes_and_the_long_258(ledger):
    assert "match_into_stored" in ledger and "258_as_284_31" in ledger


def test_hand_built_vectors_show_what_they_are_named_for(ledger):
    """Each row above is hit by the vector written for it, not only by a lucky fuzz stream."""
    for feature, name in ((("litlen_bits", 15), "many_15bit"), ("15+5_then_15+13_ones", "max_bits"),
                          ("258_as_284_31", "max_bits"), (("crossing", 16), "repeat_crosses"),
                          (("crossing", 18), "zero_run_crosses"), (("crossing", 17), "zero_run_crosses_17"),
                          ("one_dist_code_used", "one_dist_code"), ("one_dist_code_used", "one_dist_code_sym5"),
                          ("no_dist_code", "no_dist_code"), (("hclen", 5), "hclen5"),
                          (("clen_code_bits", 7), "clen_7bit"), ("match_into_stored", "lit70_empty_stored_stored65")):
        assert name in ledger[feature], (feature, name)
    for pad in range(8):
        assert any(n.startswith("stored_align_") for n in ledger[("stored_pad", pad)])
        assert "stored_align_%d" % pad in ledger["match_into_stored"]
    assert "repeat_stops_at_boundary" not in ledger[("crossing", 16)]  # the same sets, coded apart
