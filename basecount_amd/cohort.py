"""Cohort runs: many BAM files counted together in one process ("Cohort runs").

A sample of amplicon size costs microseconds of kernel time and, alone, a process start, a decode,
a launch and a handful of blocking round trips.  ``get_basecounts_many`` takes a list of files
instead: the selected reads of consecutive *regular* files are laid side by side in shared device
buffers, every (file, reference) pair becomes one segment of a virtual reference, and one
``bc_segments_rebase`` + one ``bc_pileup_segments`` (+ one ``bc_amplicons_segments`` with a BED)
count the whole group.  Everything else -- an irregular file, a file that would be a lone segment, a
failing one -- goes through ``get_basecounts`` itself, in this process, so its output and its errors
are the existing path's by construction.  Nothing here changes what ``get_basecounts``, ``run()`` or
the ``basecount`` command do.

    python -m basecount_amd.cohort [every flag of basecount] --out-dir DIR BAM [BAM ...]

writes DIR/X.tsv for input X.bam: the bytes ``python -m basecount_amd X.bam <flags>`` prints.
With ``--bgzf`` (what BASECOUNT_BGZF=1 sets, for the call) the per-position outputs are written as
BGZF, DIR/X.tsv.gz: the bytes that command prints under the switch.
"""
from __future__ import annotations

import contextlib
import io
import os
import queue
import sys
import threading
import time
from dataclasses import dataclass, field

import numpy as np

from . import device as D
from . import fmt
from . import main as M
from .bam import BamStream

INDEX_LIMIT = 1 << 32  # bc_cohort.h's BCC_INDEX_LIMIT: a shared buffer holds fewer CIGAR words / nibbles
READS_LIMIT = 1 << 31  # reads of one group (bc_segments_rebase: n_reads < 2^31)
BYTES_DEFAULT = 1 << 30  # upload budget of one group (BASECOUNT_COHORT_BYTES)
THREADS_DEFAULT = 16  # decode threads over the streams open at once (BASECOUNT_COHORT_THREADS)

# the last get_basecounts_many call's routing: "groups" one list of (path, reference) per launch,
# "single" the (path, reason) pairs that went through get_basecounts, "ops" the groups that took the
# long-read kernel shape
PLAN: dict = {"groups": [], "single": [], "ops": []}
# wall seconds of the last call by phase (the CLI's BASECOUNT_HIP_TIMING line)
TIMES: dict = {}


def byte_budget() -> int:
    v = os.environ.get("BASECOUNT_COHORT_BYTES")
    return max(1, int(v)) if v else BYTES_DEFAULT


def thread_budget() -> int:
    v = os.environ.get("BASECOUNT_COHORT_THREADS")
    return max(1, int(v)) if v else THREADS_DEFAULT


# ------------------------------------------------------------------------------- the planner
@dataclass
class FileFacts:
    """What the planner knows of one file.  ``reason``: None for a regular file, else why it is not
    (it then takes the per-file path).  ``lengths``: its requested references' lengths, one segment
    each; ``n_reads`` selected reads, ``cig_words`` CIGAR words and ``seq_bytes`` padded sequence
    bytes (a multiple of 16) to upload; ``ops``: the file's wants_ops answer."""

    path: str
    reason: str | None = None
    lengths: tuple = ()
    n_reads: int = 0
    cig_words: int = 0
    seq_bytes: int = 0
    ops: bool = False

    def virt(self) -> int:
        return sum((int(L) + 63) // 64 * 64 for L in self.lengths)

    def upload_bytes(self, want_qual: bool) -> int:
        return 4 * self.cig_words + (3 if want_qual else 1) * self.seq_bytes + 16 * self.n_reads


@dataclass
class _Run:
    files: list = field(default_factory=list)
    virt: int = 0
    reads: int = 0
    words: int = 0
    seq: int = 0
    nbytes: int = 0

    def segments(self) -> int:
        return sum(len(f.lengths) for f in self.files)


class Planner:
    """plan_cohort one file at a time (the decoder feeds it while earlier groups are on the device):
    ``add`` returns the units the new file closes, ``finish`` the last ones.  A unit is
    ("group", [facts, ...]) or ("single", facts, reason)."""

    def __init__(self, cap: int, budget: int, want_qual: bool):
        self.cap, self.budget, self.want_qual = int(cap), int(budget), bool(want_qual)
        self.run = _Run()

    def _fits_alone(self, f: FileFacts) -> str | None:
        if f.virt() > self.cap:
            return "exceeds the group's position cap"
        if f.cig_words >= INDEX_LIMIT or 2 * f.seq_bytes >= INDEX_LIMIT or f.n_reads >= READS_LIMIT:
            return "exceeds the 32-bit index budgets"
        if f.upload_bytes(self.want_qual) > self.budget:
            return "exceeds the upload budget"
        return None

    def _crosses(self, f: FileFacts) -> bool:
        r = self.run
        return bool(r.files) and (
            r.virt + f.virt() > self.cap
            or r.words + f.cig_words >= INDEX_LIMIT or 2 * (r.seq + f.seq_bytes) >= INDEX_LIMIT
            or r.reads + f.n_reads >= READS_LIMIT
            or r.nbytes + f.upload_bytes(self.want_qual) > self.budget
            or r.files[0].ops != f.ops)

    def _close(self) -> list:
        r, self.run = self.run, _Run()
        if not r.files:
            return []
        if r.segments() < 2:  # one file with one reference: nothing to share a launch with
            return [("single", r.files[0], "lone segment")]
        return [("group", r.files)]

    def add(self, f: FileFacts) -> list:
        if self.cap <= 0:
            return [("single", f, f.reason or "grouping is off")]
        reason = f.reason or (None if f.lengths else "no requested reference") or self._fits_alone(f)
        if reason is not None:  # an irregular file ends the run
            return self._close() + [("single", f, reason)]
        out = self._close() if self._crosses(f) else []
        r = self.run
        r.files.append(f)
        r.virt += f.virt()
        r.reads += f.n_reads
        r.words += f.cig_words
        r.seq += f.seq_bytes
        r.nbytes += f.upload_bytes(self.want_qual)
        return out

    def finish(self) -> list:
        return self._close()


def plan_cohort(facts, cap: int | None = None, budget: int | None = None, want_qual: bool = False):
    """The launches of a cohort: maximal runs of consecutive regular files (input order), cut where
    the sum of round_up(L, 64) would pass ``cap`` (group_cap()), the CIGAR words or 2 x the padded
    sequence bytes would reach 2^32, the reads 2^31, the upload bytes would pass ``budget``
    (BASECOUNT_COHORT_BYTES), or the files' wants_ops answers differ.  A file is never split; a run
    of one segment is not a group.  Pure: no device, no file.  Returns (groups, single): lists of
    FileFacts per group, and (FileFacts, reason) pairs, both in input order."""
    p = Planner(M.group_cap() if cap is None else cap, byte_budget() if budget is None else budget, want_qual)
    units = [u for f in facts for u in p.add(f)] + p.finish()
    return [u[1] for u in units if u[0] == "group"], [(u[1], u[2]) for u in units if u[0] == "single"]


def output_names(bams, out_dir: str, ext: str = ".tsv") -> list:
    """DIR/X.tsv for X.bam (the extension dropped, whatever it is; ``ext``: ".tsv.gz" under --bgzf);
    duplicate basenames are refused before any work starts."""
    seen, out = {}, []
    for b in bams:
        stem = os.path.splitext(os.path.basename(os.fspath(b)))[0]
        if stem in seen:
            raise ValueError(f"duplicate basename {stem!r}: {seen[stem]} and {b} would both write {stem}{ext}")
        seen[stem] = b
        out.append(os.path.join(out_dir, stem + ext))
    return out


# ------------------------------------------------------------------------------- decoding
class _Decoded:
    """One file decoded and selected on the host: its facts, and for a regular file the batch whose
    arrays are uploaded (closed once the group's copies are done)."""

    def __init__(self, path):
        self.path = path
        self.facts = FileFacts(path)
        self.stream = self.batch = self.sel = None
        self.ref_order, self.names, self.tids, self.lens = [], (), [], []
        self.lengths_t, self.nreads = (), None  # by refID: the header's lengths, the selected reads

    def close(self):
        for h in (self.batch, self.stream):
            if h is not None:
                h.close()
        self.batch = self.stream = self.sel = None


def _decode(path, references, mmq, B, nthreads) -> _Decoded:
    """Decode + select one file and decide whether it is regular (module docstring); whatever goes
    wrong here makes it irregular, and get_basecounts then reports it its own way."""
    d = _Decoded(path)
    try:
        d.stream = st = BamStream(path, nthreads)
        refs = M.get_references(st, references)
        d.ref_order, d.names, d.lengths_t = list(refs), st.references, st.lengths
        wanted = [n in refs for n in st.references]
        lens_t = np.asarray(st.lengths, np.int64)
        d.tids = [t for t, w in enumerate(wanted) if w]
        d.lens = [int(lens_t[t]) for t in d.tids]
        if not all(0 < L <= M.GROUP_MAX_LEN for L in d.lens):
            raise _Irregular("a reference is empty or longer than GROUP_MAX_LEN")
        d.batch = f = st.next_batch(B)
        if f is None:
            raise _Irregular("no records")
        more = st.next_batch(B)
        if more is not None:
            more.close()
            raise _Irregular("more than one batch")
        d.sel = sel = f.select(mmq, wanted)
        if sel.keyerror_ordinal >= 0:
            raise _Irregular("a read of an unrequested reference")
        if sel.rec.size and bool(np.any(f.rec_err[sel.rec] != 0)):
            raise _Irregular("a faulty record")
        d.nreads = np.diff(sel.ref_beg)
        p = sel.pos.astype(np.int64)
        tid = np.repeat(np.arange(len(st.references)), np.diff(sel.ref_beg))
        if bool(np.any((p < 0) | (p + sel.span > lens_t[tid]))):
            raise _Irregular("a read outside its reference")
        if not bool(np.all(M._reads_inside(sel.pos, sel.span, sel.ref_beg, lens_t))):
            raise _Irregular("unsorted within a reference")
        d.facts = FileFacts(path, None, tuple(d.lens), int(sel.pos.size), int(f.cigar.size), int(f.seq_event.size),
                            M.wants_ops(sel.cig_n))
    except _Irregular as e:
        d.facts = FileFacts(path, str(e))
    except Exception as e:  # noqa: BLE001 - the per-file path raises it again, its own way
        d.facts = FileFacts(path, f"{type(e).__name__} while decoding")
    if d.facts.reason is not None:
        d.close()
    return d


class _Irregular(Exception):
    pass


# ------------------------------------------------------------------------------- one group
def _put(ctx, buf, offset: int, a: np.ndarray) -> None:
    """Stream-ordered copy of a host array to ``offset`` bytes into a device buffer."""
    a = np.ascontiguousarray(a)
    if a.nbytes:
        assert offset + a.nbytes <= buf.nbytes
        D.check(D.lib().bc_memcpy_h2d(ctx.h, buf.ptr + offset, a.ctypes.data, a.nbytes))
        ctx._keep.append(a)  # alive until the next sync


def _run_group(ctx, scratch, files, mbq, k, nf, nf2, mode, tiles, ops, fm) -> list:
    """The group's files side by side in the scratch's batch buffers, rebased and counted in one
    launch; returns one result per segment (file order, refID order within a file) as _device_group
    gives them."""
    want_qual = mbq > 0
    n_files = len(files)
    words = np.zeros(n_files + 1, np.int64)
    seqb = np.zeros(n_files + 1, np.int64)
    rbeg = np.zeros(n_files + 1, np.int64)
    for i, d in enumerate(files):
        words[i + 1] = words[i] + d.batch.cigar.size
        seqb[i + 1] = seqb[i] + d.batch.seq_event.size
        rbeg[i + 1] = rbeg[i] + d.sel.pos.size
    n, tw, tb = int(rbeg[-1]), int(words[-1]), int(seqb[-1])
    assert tw < INDEX_LIMIT and 2 * tb < INDEX_LIMIT and n < READS_LIMIT  # the planner's cuts
    with M._phase("upload"):
        t0 = time.perf_counter()
        d_cigar, d_seq = scratch.get("b_cigar", max(4, 4 * tw)), scratch.get("b_seq", max(16, tb))
        d_qual = scratch.get("b_qual", max(4, 2 * tb)) if want_qual else None
        per = {r: scratch.get(r, max(4, 4 * n)) for r in ("b_pos", "b_cb", "b_cn", "b_sn")}
        lens, read_beg, cig_base, nib_base, span = [], [0], [], [], 0
        for i, d in enumerate(files):
            f, sel = d.batch, d.sel
            assert int(seqb[i]) % 16 == 0
            _put(ctx, d_cigar, 4 * int(words[i]), f.cigar)
            _put(ctx, d_seq, int(seqb[i]), f.seq_event)
            if want_qual:
                _put(ctx, d_qual, 2 * int(seqb[i]), f.qual)
            for role, a in (("b_pos", sel.pos), ("b_cb", sel.cig_beg), ("b_cn", sel.cig_n), ("b_sn", sel.seq_nib)):
                _put(ctx, per[role], 4 * int(rbeg[i]), a)
            for t in d.tids:  # the file's segments: its requested references in refID order
                lens.append(int(d.lengths_t[t]))
                read_beg.append(int(rbeg[i]) + int(sel.ref_beg[t + 1]))
                cig_base.append(int(words[i]))
                nib_base.append(2 * int(seqb[i]))
            if sel.span.size:
                span = max(span, int(sel.span.max()))
        n_seg = len(lens)
        assert read_beg[-1] == n
        bases = np.concatenate([np.asarray(read_beg, np.int64).view(np.uint64), np.asarray(cig_base, np.uint64),
                                np.asarray(nib_base, np.uint64)])
        d_bases = scratch.get("cohort_bases", bases.nbytes).upload(bases)
        TIMES["upload"] += time.perf_counter() - t0
    with M._phase("kernels + download"):
        t0 = time.perf_counter()
        ctx.segments_rebase(n, n_seg, d_bases.ptr, d_bases.ptr + 8 * (n_seg + 1), d_bases.ptr + 8 * (2 * n_seg + 1),
                            tw, 2 * tb, per["b_cb"].ptr, per["b_sn"].ptr)
        r = D.BcReads()
        r.n_reads = n
        r.pos, r.cig_beg, r.cig_n, r.seq_nib = (per[x].ptr for x in ("b_pos", "b_cb", "b_cn", "b_sn"))
        r.cigar, r.n_cigar_words = d_cigar.ptr, tw
        r.seq, r.seq_bytes, r.seq_layout = d_seq.ptr, max(0, tb - 16), D.BC_SEQ_EVENT
        if want_qual:
            r.qual, r.qual_bytes = d_qual.ptr, 2 * max(0, tb - 16)
        r.sorted, r.max_span = 1, min(span, 2**31 - 1)
        if fm is not None:
            fm.names = [d.names[t] for d in files for t in d.tids]
            scratch.formatter = fm
        try:
            with M._ops_shape(ctx, ops):
                res = M._device_group(ctx, r, lens, read_beg, mbq, k, nf, nf2, mode, scratch, tiles=tiles)
            bad = ctx.range_error()  # (synchronises: the files' host arrays may go)
        finally:
            scratch.formatter = None
        assert bad == -1, "a regular file's read left its reference"
        ctx.sync()
        TIMES["kernels"] += time.perf_counter() - t0
    return res


# ------------------------------------------------------------------------------- the API
def get_basecounts_many(bams, references=None, min_base_quality=0, min_mapping_quality=0, chunk_size=1000000,
                        show_n_bases=False, long_format=False, *, device=None, _mode="rows", _tiles=None, _dp=None,
                        _single=None, _emit=None):
    """``{path: result}`` in input order, where result is what ``get_basecounts(path, <the same
    arguments>)`` returns in this process -- the same keys in the same order, the arrays bit for bit
    -- or, where that call raises, the exception instance.  A failing file never stops the others.

    Consecutive *regular* files are counted together, one launch per group (``plan_cohort``); a
    file is regular when it opens, its records fit one batch of ``batch_records(chunk_size)``, the
    selection reports no read of an unrequested reference and no faulty record, every requested
    reference has 0 < L <= GROUP_MAX_LEN, and its reads are in start order inside their references.
    Every other file goes through ``get_basecounts`` (``_single(path)`` when given: the CLI's
    per-file run; ``_emit(path, result)``, when given, takes each fast-path result as soon as its
    group is done and the returned dict holds None in its place: the CLI writes and forgets it, so
    memory holds one group's results, not the cohort's).  Later files are decoded in a host thread
    while the device works, at most one group ahead.  ``PLAN`` records the routing."""
    bams = list(dict.fromkeys(os.fspath(b) for b in bams))  # (a path given twice is one key)
    PLAN["groups"], PLAN["single"], PLAN["ops"] = [], [], []
    TIMES.update(decode=0.0, upload=0.0, kernels=0.0, files=len(bams))
    kw = dict(references=references, min_base_quality=min_base_quality, min_mapping_quality=min_mapping_quality,
              chunk_size=chunk_size, show_n_bases=show_n_bases, long_format=long_format, device=device,
              _mode=_mode, _tiles=_tiles, _dp=_dp)
    results: dict = {}

    def single(path, reason):
        PLAN["single"].append((path, reason))
        try:
            results[path] = _single(path) if _single is not None else M.get_basecounts(path, **kw)
        except Exception as e:  # noqa: BLE001 - the file's result
            results[path] = e

    text = _mode == "text"
    mode = "rows" if text else _mode
    try:
        mbq, B = int(min_base_quality), M.batch_records(chunk_size)
        fast = 0 <= mbq < (1 << 32) and mode in ("rows", "summary") and M.group_cap() > 0
        if fast and _tiles is not None and mode != "summary":
            fast = False
        dp = int(_dp) if text else None
    except Exception:  # noqa: BLE001 - arguments get_basecounts itself must refuse
        fast = False
    if not fast:
        for b in bams:
            single(b, "grouping is off" if M.group_cap() <= 0 else "arguments the fast path does not take")
        return {b: results[b] for b in bams}

    k = 6 if show_n_bases else 5
    nf, nf2 = M.norm_factors(k)
    planner = Planner(M.group_cap(), byte_budget(), mbq > 0)
    units: queue.Queue = queue.Queue()
    slots = threading.Semaphore(2)  # the unit on the device and the one decoded ahead of it
    stop = threading.Event()
    threads = thread_budget()

    def producer():
        """Decode in input order and hand every closed unit to the device loop.  A slot is taken
        when a run starts, so at most one group is decoded ahead of the one being counted."""
        held = {}  # path -> _Decoded of the open run's files
        open_run = False
        try:
            for path in bams:
                if stop.is_set():
                    break
                if not open_run:
                    slots.acquire()
                    open_run = True
                t0 = time.perf_counter()
                d = _decode(path, references, min_mapping_quality, B, threads)
                TIMES["decode"] += time.perf_counter() - t0
                held[path] = d
                closed = planner.add(d.facts)
                for j, u in enumerate(closed):
                    if j:  # a second unit closed by the same file: it needs a slot of its own
                        slots.acquire()
                    units.put(_bind(u, held))
                if closed and planner.run.files:  # the file itself opened the next run
                    slots.acquire()
                open_run = bool(planner.run.files)  # (else its slot went with the last unit)
            for u in planner.finish():  # (the open run's slot goes with it)
                units.put(_bind(u, held))
        except BaseException as e:  # noqa: BLE001 - raised on the caller's thread
            units.put(("error", e))
        finally:
            for d in held.values():
                d.close()
            units.put(None)

    def _bind(u, held):
        if u[0] == "group":
            return ("group", [held.pop(f.path) for f in u[1]])
        held.pop(u[1].path).close()
        return u

    kept_before = set(M._KEPT)
    ctx = scratch = None
    th = threading.Thread(target=producer, name="cohort-decode", daemon=True)
    th.start()
    try:
        while True:
            u = units.get()
            if u is None:
                break
            if u[0] == "error":
                raise u[1]
            try:
                if u[0] == "single":
                    single(u[1].path, u[2])
                    continue
                files = u[1]
                try:
                    if ctx is None:
                        ctx = M.context(device)
                        M._KEPT.add(ctx.device)  # the per-file calls in between leave the scratch in place
                    scratch = M._scratch(ctx)
                    tiles = None
                    if _tiles is not None:
                        got = [_tiles(d.names[t]) for d in files for t in d.tids]
                        if any(g is None for g in got) or any(list(g) != list(got[0]) for g in got):
                            tiles = False  # the BED does not load (or differs by reference): per file
                        else:
                            tiles = [(int(a), int(b)) for a, b in got[0]]
                    names = [d.names[t] for d in files for t in d.tids]
                    fm = None
                    if tiles is not False and text:
                        M.PLAN["format"] = {"device": 0, "host": 0, "declined": []}
                        if D.fmt_supported(dp, names):
                            fm = M._DeviceFormatter(ctx, scratch, k, dp, long_format)
                    if tiles is False:
                        res = None
                    else:
                        ops = files[0].facts.ops
                        res = _run_group(ctx, scratch, files, mbq, k, nf, nf2, mode, tiles, ops, fm)
                        group = [(d.path, d.names[t]) for d in files for t in d.tids]
                        PLAN["groups"].append(group)
                        if ops:
                            PLAN["ops"].append(group)
                finally:
                    for d in files:
                        d.close()
                if res is None:
                    for d in files:
                        single(d.path, "the BED file does not load")
                    continue
                it = iter(res)
                for d in files:
                    by_tid = {t: next(it) for t in d.tids}
                    out = {}
                    for ref in d.ref_order:
                        t = d.names.index(ref)
                        r, nr = by_tid[t], int(d.nreads[t])
                        if text:
                            if isinstance(r, M.RefData):  # not covered or declined: the host formatter
                                r = M.bgzf_text(fmt.rows_text(ref, r.counts[:k], r.pc, r.ent, r.sec, dp, long_format),
                                                k if long_format else 1)
                            out[ref] = {"text": r, "num_reads": nr}
                        elif mode == "rows":
                            out[ref] = {"rows": M.Rows(ref, r, long_format), "num_reads": nr}
                        else:
                            out[ref] = {"summary": r, "num_reads": nr, "length": int(d.lengths_t[t])}
                    if _emit is not None:
                        _emit(d.path, out)
                        out = None
                    results[d.path] = out
            finally:
                slots.release()
    finally:
        stop.set()
        while th.is_alive():  # let a blocked producer through, and close what it still holds
            slots.release()
            try:
                u = units.get(timeout=0.05)
            except queue.Empty:
                continue
            if u and u[0] == "group":
                for d in u[1]:
                    d.close()
        th.join()
        while not units.empty():
            u = units.get()
            if u and u[0] == "group":
                for d in u[1]:
                    d.close()
        M._KEPT.clear()
        M._KEPT.update(kept_before)
        if M._DEFERRED is None:
            M.release_device_memory(only_unkept=True)
    TIMES["groups"], TIMES["singles"] = len(PLAN["groups"]), len(PLAN["single"])
    return {b: results[b] for b in bams}


# ------------------------------------------------------------------------------- the CLI
def build_parser():
    """basecount's own parser (every flag, same spelling and checks) taking several BAM files, plus
    --out-dir and --bam-list."""
    parser = M.build_parser()
    parser.prog = "python -m basecount_amd.cohort"
    for a in parser._actions:
        if a.dest == "bam":
            a.dest, a.nargs, a.metavar = "bams", "*", "BAM"
            a.help = "Paths to BAM files (index files are not required)"
    parser.add_argument("--out-dir", required=True, metavar="DIR",
                        help="Directory the outputs are written to: DIR/X.tsv for input X.bam")
    parser.add_argument("--bam-list", default=None, metavar="FILE", help="A file of BAM paths, one per line")
    parser.add_argument("--bgzf", action="store_true",
                        help="Write the per-position outputs as BGZF: DIR/X.tsv.gz (summaries stay plain text)")
    return parser


@contextlib.contextmanager
def _stdout_to(path):
    """sys.stdout writing to ``path`` as the console script's does to a pipe (UTF-8 text over a
    binary layer: fmt.write_bytes and print() both end up in the file, in order)."""
    with open(path, "wb") as raw:
        txt = io.TextIOWrapper(raw, encoding="utf-8", write_through=True)
        try:
            with contextlib.redirect_stdout(txt):
                yield
                txt.flush()
        finally:
            txt.flush()
            txt.detach()


def run(argv=None) -> int:
    """The command: returns the exit status (1 if any file failed)."""
    args = build_parser().parse_args(argv)
    if not args.bgzf:
        return _run(args)
    before = os.environ.get("BASECOUNT_BGZF")
    os.environ["BASECOUNT_BGZF"] = "1"  # what the switch sets, for the duration of the call
    try:
        return _run(args)
    finally:
        if before is None:
            del os.environ["BASECOUNT_BGZF"]
        else:
            os.environ["BASECOUNT_BGZF"] = before


def _run(args) -> int:
    from . import dist

    if dist.env()[0] > 1:
        print("basecount cohort: WORLD_SIZE > 1 is not supported (files are not sharded over ranks)", file=sys.stderr)
        return 2
    references = M.handle_arg(args.references, "references")
    mbq = int(M.handle_arg(args.min_base_quality, "min-base-quality", default=0, provided_once=True))
    mmq = int(M.handle_arg(args.min_mapping_quality, "min-mapping-quality", default=0, provided_once=True))
    chunk_size = int(M.handle_arg(args.chunk_size, "chunk-size", default=1000000, provided_once=True))
    bed = M.handle_arg(args.summarise_with_bed, "bed", provided_once=True)
    dp = int(M.handle_arg(args.decimal_places, "decimal_places", default=3, provided_once=True))
    bams = list(args.bams)
    if args.bam_list is not None:
        with open(args.bam_list) as fh:
            bams += [ln.strip() for ln in fh if ln.strip()]
    if not bams:
        print("basecount cohort: no BAM file given", file=sys.stderr)
        return 2
    try:
        gz = (not args.summarise) and bed is None and M.device_bgzf_on()
        outs = dict(zip(bams, output_names(bams, args.out_dir, ".tsv.gz" if gz else ".tsv")))
    except ValueError as e:
        print(f"basecount cohort: {e}", file=sys.stderr)
        return 2
    os.makedirs(args.out_dir, exist_ok=True)
    timing = os.environ.get("BASECOUNT_HIP_TIMING") not in (None, "", "0")
    t_start = time.perf_counter()
    t_write = [0.0]
    rows = (not args.summarise) and bed is None
    text = rows and M.device_format_on()

    def per_file(path):
        """basecount's own run of one file with its stdout in the file's output: what it prints up
        to a failure stays there, and the failure is the file's result."""
        one = build_args(args, path)
        with _stdout_to(outs[path]):
            M._run(one, references, mbq, mmq, chunk_size, bed, dp, None)
        return None

    windows = []  # the BED's windows, parsed once: the same file answers the same for every reference

    def tiles(ref):
        if not windows:
            try:
                windows.append([(t[2]["inside_start"], t[2]["inside_end"]) for t in M.load_scheme(bed)])
            except Exception:  # noqa: BLE001 - the per-file run raises it where basecount does
                windows.append(None)
        return windows[0]

    kw = dict(references=references, min_base_quality=mbq, min_mapping_quality=mmq, chunk_size=chunk_size,
              show_n_bases=args.show_n_bases, long_format=args.long_format, _single=per_file)
    if text:
        kw.update(_mode="text", _dp=dp)
    elif not rows:
        kw.update(_mode="summary", _tiles=tiles if bed is not None else None)
    def write(path, r):
        """A fast-path file's output, written as soon as its group is done."""
        t0 = time.perf_counter()
        with _stdout_to(outs[path]):
            if rows and M.device_bgzf_on():
                from . import bgzf

                with bgzf.Writer() as w:
                    w.write(("\t".join(M._columns(args.show_n_bases, args.long_format)) + "\n").encode())
                    for ref, v in r.items():
                        w.write_blocks(v["text"])
            elif rows:
                print("\t".join(M._columns(args.show_n_bases, args.long_format)))
                for ref, v in r.items():
                    if text:
                        fmt.write_bytes(v["text"])
                    else:
                        d = v["rows"].d
                        fmt.write_bytes(fmt.rows_text(ref, d.counts[: v["rows"].k], d.pc, d.ent, d.sec, dp,
                                                      args.long_format))
            else:
                for ref, v in r.items():
                    M._print_summary(ref, v["summary"], v["length"], v["num_reads"], dp, bed, None)
        t_write[0] += time.perf_counter() - t0

    res = get_basecounts_many(bams, _emit=write, **kw)
    failed = [(path, res[path]) for path in bams if isinstance(res[path], Exception)]
    for path, _ in failed:
        if not os.path.exists(outs[path]):
            open(outs[path], "wb").close()
    for path, e in failed:
        print(f"{path}: {type(e).__name__}: {e}", file=sys.stderr)
    if timing:
        t = TIMES
        print(f"basecount cohort: {t.get('files', 0)} files, {t.get('groups', 0)} groups, {t.get('singles', 0)} singles; "
              f"decode {t.get('decode', 0.0) * 1e3:.2f} ms, upload {t.get('upload', 0.0) * 1e3:.2f} ms, "
              f"kernels + download {t.get('kernels', 0.0) * 1e3:.2f} ms, format + write {t_write[0] * 1e3:.2f} ms, "
              f"wall {(time.perf_counter() - t_start) * 1e3:.2f} ms", file=sys.stderr)
    return 1 if failed else 0


def build_args(args, path):
    """The parsed arguments of `basecount PATH <the same flags>`."""
    import copy

    one = copy.copy(args)
    one.bam = path
    return one


if __name__ == "__main__":
    sys.exit(run())
