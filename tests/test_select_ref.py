"""The yardstick of the device read selection: select_ref (tests/select_inputs.py) equals
bcio_select array by array on the golden files, its sorted / inside bits equal main._reads_inside,
and main.wants_ops_counts equals main.wants_ops.  The host twin and the kernels are then measured
against select_ref (tests/test_select_host.py, tests/test_gpu_select.py)."""
import os

import numpy as np
import pytest

import select_inputs as S
from basecount_amd import main
from basecount_amd.bam import BamFile

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"c1": "c1.bam", "edge": "edge.bam", "mixed": "mixed.bam", "err_order": "err_order.bam", "ont": "ont/ont.bam"}


@pytest.fixture(scope="module")
def files():
    out = {}
    for name, rel in FILES.items():
        out[name] = BamFile(os.path.join(GOLDEN, rel))
    yield out
    for f in out.values():
        f.close()


def record_arrays(f):
    return {k: getattr(f, k) for k, _, _ in S.REC_FIELDS}


@pytest.mark.parametrize("name", sorted(FILES))
@pytest.mark.parametrize("every_second", [False, True])
def test_select_ref_equals_bcio_select(files, name, every_second):
    f = files[name]
    nr = len(f.references)
    ref_sel = np.ones(nr, np.uint8)
    if every_second:
        ref_sel[1::2] = 0
    a = record_arrays(f)
    for mmq in (-1, 0, 30, 255, 256):
        want = f.select(mmq, ref_sel)
        got = S.select_ref(a, mmq, ref_sel, f.lengths)
        what = "%s mmq=%d every_second=%s" % (name, mmq, every_second)
        for k in ("n_accepted", "keyerror_ordinal", "keyerror_rec"):
            assert got[k] == getattr(want, k), "%s: %s" % (what, k)
        assert np.array_equal(got["ref_beg"], want.ref_beg), what
        for k, dt in S.READ_ARRAYS:
            w = getattr(want, k)
            assert got[k].dtype == w.dtype and np.array_equal(got[k], w), "%s: %s" % (what, k)
        # the two bits are main._reads_inside's answer
        both = (got["flags"] & 3) == 3
        inside = main._reads_inside(want.pos, want.span, want.ref_beg, np.asarray(f.lengths, np.int64))
        assert np.array_equal(both, inside), what
        assert np.array_equal(got["n_reads"], np.diff(want.ref_beg)), what


def test_the_goldens_are_what_the_cli_tests_rely_on(files):
    """c1, mixed and ont: their mapped reads' tids never decrease and no record has a fault bit, so
    a run with the device selection never falls back on them; edge and err_order are not grouped."""
    for name in ("c1", "mixed", "ont"):
        f = files[name]
        r = S.select_ref(record_arrays(f), 0, np.ones(len(f.references), np.uint8), f.lengths)
        assert r["status"] == S.ST_OK and r["n_selected"] > 0, name
        assert not f.rec_err.any(), name
        assert r["keyerror_ordinal"] == -1, name
    for name in ("edge", "err_order"):
        f = files[name]
        r = S.select_ref(record_arrays(f), 0, np.ones(len(f.references), np.uint8), f.lengths)
        assert r["status"] == S.ST_UNGROUPED, name


def test_wants_ops_counts_equals_wants_ops(monkeypatch):
    rng = np.random.default_rng(5)
    arrays = [np.zeros(0, np.uint32), np.array([8], np.uint32), np.array([9], np.uint32),
              np.array([9, 8], np.uint32), np.array([9, 9, 8, 8], np.uint32), np.array([10, 8], np.uint32),
              np.array([2**32 - 1] * 3 + [1], np.uint32)]
    for _ in range(300):
        n = int(rng.integers(1, 400))
        hi = int(rng.choice([9, 10, 12, 18, 40, 2000]))
        arrays.append(rng.integers(1, hi + 1, n).astype(np.uint32))
    for v in (None, "", "0", "1", "auto"):
        if v is None:
            monkeypatch.delenv("BASECOUNT_LONG_READS", raising=False)
        else:
            monkeypatch.setenv("BASECOUNT_LONG_READS", v)
        seen = set()
        for c in arrays:
            a = main.wants_ops(c)
            b = main.wants_ops_counts(c.size, int((c > 8).sum()), int(c.astype(np.uint64).sum()))
            assert a == b, (v, c[:8], c.size)
            seen.add(a)
        if v in (None, "", "auto"):
            assert seen == {True, False}
