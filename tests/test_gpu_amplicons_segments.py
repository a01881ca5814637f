"""bc_amplicons_segments on the GPU: the same windows on every segment of a virtual reference, each
clipped to its own segment.  Every output is compared bit for bit with the oracle's numpy
restatement (oracle.amplicons) over the segment's slice and with bc_amplicons run on that slice;
the pads hold values that would change any mean or median they leaked into, and every segment's
values live on a scale of their own, so a neighbour's would too."""
import numpy as np
import pytest

import oracle as O
from basecount_amd import device as D

pytestmark = pytest.mark.gpu

SEG_LENS = [1, 63, 64, 65, 300, 513, 700, 8193]
# clipped at 0; one position; 512 positions (the sort path); 513 (the select path); clipped at L;
# wholly past every segment but the last; lo > hi; a whole buffer + 1
WINDOWS = [(-5, 3), (0, 0), (10, 521), (10, 522), (250, 10000), (9000, 9100), (5, 4), (0, 8192)]


@pytest.fixture(scope="module")
def ctx():
    return D.Context(0)


@pytest.fixture(scope="module")
def layout():
    rng = np.random.default_rng(515)
    lens = np.array(SEG_LENS, np.int64)
    voff = D.segments_layout(lens)
    Lv = int(voff[-1])
    # the pads: values no segment holds, far above all of them
    cov = np.full(Lv, 1 << 30, np.int32)
    ent = np.full(Lv, 1.0e6)
    sec = np.full(Lv, 3.0e6)
    for i, L in enumerate(SEG_LENS):
        sl = slice(int(voff[i]), int(voff[i]) + L)
        cov[sl] = rng.integers(0, 50, L) + 1000 * i  # (ties within a segment, none across segments)
        ent[sl] = rng.integers(0, 7, L) / 7.0 + i if i % 2 else rng.random(L) + i
        sec[sl] = rng.random(L) + 2 * i
    return dict(lens=lens, voff=voff, Lv=Lv, cov=cov, ent=ent, sec=sec)


@pytest.fixture(scope="module")
def device_run(ctx, layout):
    """One bc_amplicons_segments launch over all (segment, window) pairs, and bc_amplicons per slice."""
    n, nt, Lv = len(SEG_LENS), len(WINDOWS), layout["Lv"]
    lo = np.array([w[0] for w in WINDOWS], np.int64)
    hi = np.array([w[1] for w in WINDOWS], np.int64)
    dc, de, ds = (ctx.alloc(4 * Lv).upload(layout["cov"]), ctx.alloc(8 * Lv).upload(layout["ent"]),
                  ctx.alloc(8 * Lv).upload(layout["sec"]))
    tab = np.concatenate([layout["lens"], layout["voff"], lo, hi])
    dt = ctx.alloc(tab.nbytes).upload(tab)
    p_len, p_voff, p_lo, p_hi = dt.ptr, dt.ptr + 8 * n, dt.ptr + 8 * (2 * n + 1), dt.ptr + 8 * (2 * n + 1 + nt)
    out = ctx.alloc(48 * n * nt + 64)
    assert D.lib().bc_memset(ctx.h, out.ptr, 0x5A, out.nbytes) == 0
    ctx.amplicons_segments(dc.ptr, de.ptr, ds.ptr, n, p_len, p_voff, p_lo, p_hi, nt, out.ptr)
    raw = out.download(np.float64, 6 * n * nt + 8)
    assert np.all(raw[6 * n * nt:].view(np.uint8) == 0x5A)  # nothing past the last pair
    got = raw[:6 * n * nt].reshape(n, nt, 6)
    alone = np.zeros((n, nt, 6))
    one = ctx.alloc(48 * nt)
    for i, L in enumerate(SEG_LENS):
        v = int(layout["voff"][i])
        ctx.amplicons(dc.ptr + 4 * v, de.ptr + 8 * v, ds.ptr + 8 * v, L, p_lo, p_hi, nt, one.ptr)
        alone[i] = one.download(np.float64, 6 * nt).reshape(nt, 6)
    return got, alone


@pytest.mark.parametrize("seg", range(len(SEG_LENS)), ids=[f"L{L}" for L in SEG_LENS])
def test_windows_equal_numpy_and_bc_amplicons_on_the_slice(layout, device_run, seg):
    got, alone = device_run
    L, v = SEG_LENS[seg], int(layout["voff"][seg])
    sl = slice(v, v + L)
    exp = O.amplicons(layout["cov"][sl], layout["ent"][sl], layout["sec"][sl], WINDOWS)
    for t, e in enumerate(exp):
        assert got[seg, t].tolist() == [float(x) for x in e], (L, WINDOWS[t])
        assert got[seg, t].tobytes() == alone[seg, t].tobytes(), (L, WINDOWS[t])


def test_the_windows_take_every_path(layout):
    """The cases are what they are named for: both median paths, clipped and empty windows."""
    n = {(L, w): max(0, min(w[1], L - 1) - max(w[0], 0) + 1) for L in SEG_LENS for w in WINDOWS}
    assert n[(8193, (10, 521))] == 512 and n[(8193, (10, 522))] == 513 and n[(8193, (0, 8192))] == 8193
    assert n[(700, (250, 10000))] == 450 and n[(8193, (9000, 9100))] == 0 and n[(1, (-5, 3))] == 1
    assert all(n[(L, (5, 4))] == 0 for L in SEG_LENS)
    assert all(v % 64 == 0 for v in layout["voff"].tolist())


def test_zero_windows_is_a_no_op(ctx):
    ctx.amplicons_segments(None, None, None, 3, None, None, None, None, 0, None)
    ctx.sync()
