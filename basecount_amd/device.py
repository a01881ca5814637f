"""ctypes bindings for ``libbasecount_hip.so`` (``include/basecount_hip.h``).

``Context`` wraps one ``bc_ctx`` (device + stream); ``DeviceBuffer`` is a library-owned HBM
allocation; ``DeviceReads`` is an uploaded read batch (``bc_reads``).  Pointers may also come
from another allocator (e.g. ``torch.Tensor.data_ptr()``) — the C-ABI only sees addresses.

There is no CPU fallback: if the library or a gfx950 device is missing, the calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._native import _libs, _load

BC_E_ARG, BC_E_HIP, BC_E_RANGE, BC_E_NODEV, BC_E_COMM = -1, -2, -3, -4, -5
COMM_ID_BYTES = 128  # BC_COMM_ID_BYTES
BC_SEQ_BAM, BC_SEQ_EVENT = 0, 1
SHAPES = {"auto": 0, "tile": 1, "rc": 2, "tile_no_solo": 3, "ops": 4}  # BC_SHAPE_*
KERNEL_NAMES = ("count", "stats", "rc", "pileup", "summary", "amplicons", "index", "solo", "sort")  # BC_K_* ids
BC_INDEX_RUNS, BC_INDEX_TILES, BC_INDEX_AUTO = 1, 2, 4
KERNEL_IDS = len(KERNEL_NAMES)


class BcReads(C.Structure):
    _fields_ = [
        ("n_reads", C.c_int64),
        ("pos", C.c_void_p),
        ("cig_beg", C.c_void_p),
        ("cig_n", C.c_void_p),
        ("seq_nib", C.c_void_p),
        ("cigar", C.c_void_p),
        ("n_cigar_words", C.c_int64),
        ("seq", C.c_void_p),
        ("seq_bytes", C.c_int64),
        ("qual", C.c_void_p),
        ("qual_bytes", C.c_int64),
        ("sorted", C.c_int32),
        ("max_span", C.c_int32),
        ("max_end", C.c_int64),
        ("seq_layout", C.c_int32),  # BC_SEQ_BAM 0 / BC_SEQ_EVENT 1
        ("run_chunks", C.c_int32),
        ("tile_reads", C.c_void_p),  # optional per-tile read ranges (bc_reads_upload)
        ("n_tiles", C.c_int64),
        ("read_runs", C.c_void_p),  # optional run records, 4 words per read (bc_reads_upload)
        ("index_tag", C.c_uint64),  # the batch the index was built for (0: none)
    ]


class BcZBlock(C.Structure):
    """bc_zblock (= bcio_zblock): one BGZF block's raw-DEFLATE bytes and where they inflate to."""
    _fields_ = [("coff", C.c_uint64), ("clen", C.c_uint32), ("isize", C.c_uint32), ("uoff", C.c_uint64)]


class BcBamBatch(C.Structure):
    """bc_bam_batch: what bc_bam_index found (status != 0: the fill is declined)."""
    _fields_ = [("n", C.c_int64), ("used", C.c_uint64), ("cigar_words", C.c_uint64), ("seq_bytes", C.c_uint64),
                ("status", C.c_int32), ("reserved", C.c_int32), ("err_off", C.c_uint64), ("segments", C.c_int64),
                ("repaired", C.c_int64), ("raw_bytes", C.c_uint64), ("seg_bytes", C.c_uint64)]


# bc_bam_arrays' device arrays: name, element type, elements for (n, cigar_words, seq_bytes)
BAM_ARRAYS = (
    ("tid", np.int32, lambda n, cw, sb: n), ("pos", np.int32, lambda n, cw, sb: n),
    ("flag", np.uint16, lambda n, cw, sb: n), ("mapq", np.uint8, lambda n, cw, sb: n),
    ("l_seq", np.int32, lambda n, cw, sb: n), ("qstart", np.int32, lambda n, cw, sb: n),
    ("qend", np.int32, lambda n, cw, sb: n), ("rec_err", np.uint32, lambda n, cw, sb: n),
    ("ref_span", np.int64, lambda n, cw, sb: n), ("cig_off", np.uint64, lambda n, cw, sb: n + 1),
    ("seq_off", np.uint64, lambda n, cw, sb: n + 1), ("cigar", np.uint32, lambda n, cw, sb: cw),
    ("seq", np.uint8, lambda n, cw, sb: sb), ("seq_event", np.uint8, lambda n, cw, sb: seq_event_bytes(sb)),
    ("qual", np.uint8, lambda n, cw, sb: 2 * sb),
)


class BcBamArrays(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in BAM_ARRAYS] + [
        ("n_cap", C.c_int64), ("cigar_cap", C.c_uint64), ("seq_cap", C.c_uint64)]


class BcSelHeader(C.Structure):
    """bc_sel_header: what bc_bam_select found (status != 0: declined, select on the host)."""
    _fields_ = [("status", C.c_int32), ("err_or", C.c_uint32), ("n_accepted", C.c_int64), ("n_selected", C.c_int64),
                ("keyerror_rec", C.c_int64), ("keyerror_ordinal", C.c_int64), ("reserved", C.c_int64 * 3)]


SEL_HEADER_DTYPE = np.dtype([("status", "<i4"), ("err_or", "<u4"), ("n_accepted", "<i8"), ("n_selected", "<i8"),
                             ("keyerror_rec", "<i8"), ("keyerror_ordinal", "<i8"), ("reserved", "<i8", (3,))])  # 64 bytes
# bc_sel_arrays' device arrays, in the struct's order: per selected read, then per reference
SEL_READ_ARRAYS = (("pos", np.int32), ("cig_beg", np.uint32), ("cig_n", np.uint32), ("seq_nib", np.uint32),
                   ("qlen", np.uint32), ("span", np.int64), ("rec", np.int64), ("ordinal", np.int64))
SEL_REF_ARRAYS = (("ref_beg", np.int64), ("max_span", np.int64), ("max_end", np.int64), ("n_reads", np.int64),
                  ("n_complex", np.int64), ("sum_ops", np.uint64), ("err_or", np.uint32), ("flags", np.uint32))
SEL_STATUS = ("ok", "ungrouped", "too_large")  # BC_SEL_*
SEL_SORTED, SEL_INSIDE = 1, 2


class BcSelArrays(C.Structure):
    _fields_ = ([(name, C.c_void_p) for name, _ in SEL_READ_ARRAYS] + [("n_cap", C.c_int64)]
                + [(name, C.c_void_p) for name, _ in SEL_REF_ARRAYS] + [("ref_cap", C.c_int64), ("header", C.c_void_p)])


def sel_layout(n_cap: int, ref_cap: int) -> tuple:
    """One buffer for bc_bam_select's outputs: ({name: byte offset}, bytes of the leading part the
    host downloads (the header and the per-reference arrays), total bytes)."""
    off, at = {"header": 0}, 256
    for name, dt in SEL_REF_ARRAYS:
        off[name] = at
        at += (np.dtype(dt).itemsize * (ref_cap + 1) + 255) // 256 * 256
    small = at
    for name, dt in SEL_READ_ARRAYS:
        off[name] = at
        at += (np.dtype(dt).itemsize * max(1, n_cap) + 255) // 256 * 256
    return off, small, at


def sel_arrays(base: int, n_cap: int, ref_cap: int) -> BcSelArrays:
    """bc_sel_arrays pointing into a buffer of sel_layout(n_cap, ref_cap) at device address base."""
    off, _, _ = sel_layout(n_cap, ref_cap)
    a = BcSelArrays()
    for name, o in off.items():
        setattr(a, name, base + o)
    a.n_cap, a.ref_cap = int(n_cap), int(ref_cap)
    return a


def bam_select_bytes(n: int, n_refs: int) -> int:
    """bc_bam_select_bytes: the work buffer of bc_bam_select."""
    b = C.c_size_t(0)
    check(lib().bc_bam_select_bytes(int(n), int(n_refs), C.byref(b)))
    return int(b.value)


class BcFmtArgs(C.Structure):
    """bc_fmt_args: the device arrays bc_fmt_rows prints and the segment table that says how."""
    _fields_ = [("counts", C.c_void_p), ("pc", C.c_void_p), ("ent", C.c_void_p), ("sec", C.c_void_p),
                ("stride", C.c_int64), ("n", C.c_int64), ("segs", C.c_void_p), ("n_seg", C.c_int64),
                ("names", C.c_void_p), ("names_bytes", C.c_int64), ("k", C.c_int32), ("dp", C.c_int32),
                ("long_format", C.c_int32), ("reserved", C.c_int32)]


FMT_HEADER_DTYPE = np.dtype([("status", "<i4"), ("reserved0", "<i4"), ("total_bytes", "<i8"), ("declined_pos", "<i8"),
                             ("reserved", "<i8", (5,))])  # bc_fmt_header, 64 bytes
FMT_SEG_DTYPE = np.dtype([("beg", "<i8"), ("len", "<i8"), ("pos0", "<i8"), ("name_off", "<i4"),
                          ("name_len", "<i4")])  # bc_fmt_seg, 32 bytes
FMT_STATUS = ("ok", "too_small", "value")  # BC_FMT_*
FMT_OK, FMT_TOO_SMALL, FMT_VALUE = 0, 1, 2
FMT_MAX_DP, FMT_MAX_NAME = 4, 255


def fmt_supported(dp: int, names) -> bool:
    """Whether bc_fmt_rows covers these decimal places and reference names (printed values outside its
    cover are found by the kernels: BC_FMT_VALUE)."""
    return 0 <= int(dp) <= FMT_MAX_DP and all(len(n.encode()) <= FMT_MAX_NAME for n in names)


def fmt_rows_bytes(n: int, n_seg: int) -> tuple:
    """bc_fmt_rows_bytes: (bytes of the work buffer, bytes of the header + seg_off)."""
    w, o = C.c_size_t(0), C.c_size_t(0)
    check(lib().bc_fmt_rows_bytes(int(n), int(n_seg), C.byref(w), C.byref(o)))
    return int(w.value), int(o.value)


def fmt_table(segs) -> tuple:
    """The segment table and the names array of bc_fmt_rows from (beg, len, pos0, name) tuples."""
    tab = np.zeros(len(segs), FMT_SEG_DTYPE)
    blob, at = [], 0
    for i, (beg, ln, pos0, name) in enumerate(segs):
        b = name if isinstance(name, bytes) else name.encode()
        tab[i] = (beg, ln, pos0, at, len(b))
        blob.append(b)
        at += len(b)
    return tab, np.frombuffer(b"".join(blob) + b"\0", np.uint8)


DFL_HEADER_DTYPE = np.dtype([("status", "<i4"), ("n_stored", "<i4"), ("n_blocks", "<i8"), ("total_bytes", "<i8"),
                             ("text_bytes", "<i8"), ("reserved", "<i8", (4,))])  # bc_dfl_header, 64 bytes
DFL_STATUS = ("ok", "too_small", "gated", "offsets")  # BC_DFL_*
DFL_OK, DFL_TOO_SMALL, DFL_GATED, DFL_OFFSETS = 0, 1, 2, 3
DFL_BLOCK = 65280  # input bytes of a BGZF block


def bgzf_deflate_bytes(text_cap: int, n_spans: int) -> tuple:
    """bc_bgzf_deflate_bytes: (bytes of the work buffer, bytes of the header + span_coff)."""
    w, o = C.c_size_t(0), C.c_size_t(0)
    check(lib().bc_bgzf_deflate_bytes(int(text_cap), int(n_spans), C.byref(w), C.byref(o)))
    return int(w.value), int(o.value)


def bgzf_deflate_host(text, span_off=None, nthreads: int = 16) -> tuple:
    """bc_bgzf_deflate_host: (compressed bytes as uint8, span_coff) of a bytes-like text cut at span_off
    (default: one span), the bytes bc_bgzf_deflate writes; no device is touched, no EOF block added."""
    t = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
    off = np.ascontiguousarray([0, t.size] if span_off is None else span_off, np.int64)
    n = off.size - 1
    src = t if t.size else np.zeros(1, np.uint8)
    # a fixed-code block is below its input + 5 + 26 bytes (the stored fallback), a span adds a cut
    cap = int(t.size + 31 * (t.size // DFL_BLOCK + n) + 64)
    comp, coff, total = np.empty(cap, np.uint8), np.zeros(n + 1, np.int64), C.c_int64(0)
    rc = lib().bc_bgzf_deflate_host(src.ctypes.data, off.ctypes.data, n, comp.ctypes.data, cap, coff.ctypes.data,
                                    C.byref(total), int(nthreads))
    if rc < 0:
        check(rc)
    if rc != DFL_OK:
        raise ValueError("bc_bgzf_deflate_host: " + DFL_STATUS[rc])
    return comp[:total.value], coff


BAM_STATUS = ("ok", "partial_len", "partial", "short", "neg_lseq", "fields", "too_large", "repairs", "internal")  # BC_BAM_*


ZBLOCK_DTYPE = np.dtype([("coff", "<u8"), ("clen", "<u4"), ("isize", "<u4"), ("uoff", "<u8")])  # 24 bytes


class BcPlan(C.Structure):
    _fields_ = [
        ("kernel", C.c_int32),  # BC_PLAN_RC 0 / BC_PLAN_SOLO 1 / BC_PLAN_TILES 2
        ("waves_per_tile", C.c_int32),
        ("block_threads", C.c_int32),
        ("lds_bytes", C.c_int32),
        ("blocks", C.c_int64),
        ("blocks_per_cu", C.c_int32),  # -1: no device to ask
        ("tiles_per_wave", C.c_int32),  # BC_PLAN_SOLO: tiles per wave of bc_pileup's sweep; else 0
        ("reads_per_tile", C.c_double),
    ]


PLAN_KERNELS = ("rc", "solo", "tiles")  # BC_PLAN_*
OPS_PASSES_MAX = 16  # BC_OPS_PASSES_MAX


class BcOpsPlan(C.Structure):
    _fields_ = [("reads_per_block", C.c_int32), ("window", C.c_int32), ("passes_max", C.c_int32),
                ("reserved", C.c_int32), ("blocks", C.c_int64)]
INSTANCES = {"auto": 0, "general": 1, "lean": 2, "slice": 4}  # BC_INSTANCE_* (3 is not a value)


class BcLaunchInfo(C.Structure):
    _fields_ = [
        ("kernel", C.c_int32),
        ("lean", C.c_int32),
        ("waves_per_tile", C.c_int32),
        ("block_threads", C.c_int32),
        ("lds_bytes", C.c_int32),
        ("blocks_per_cu", C.c_int32),  # -1: no device to ask
        ("blocks", C.c_int64),
    ]


class BcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


def lib() -> C.CDLL:
    L = _libs.get("libbasecount_hip.so")
    if L is not None:
        return L
    L = _load("libbasecount_hip.so")
    vp, i64, u32, dbl = C.c_void_p, C.c_int64, C.c_uint32, C.c_double
    sig = {
        "bc_last_error": ([], C.c_char_p),
        "bc_abi_version": ([], C.c_int),
        "bc_build_info": ([], C.c_char_p),
        "bc_device_count": ([C.POINTER(C.c_int)], C.c_int),
        "bc_ctx_create": ([C.c_int, vp, C.POINTER(vp)], C.c_int),
        "bc_ctx_destroy": ([vp], C.c_int),
        "bc_ctx_release_scratch": ([vp], C.c_int),
        "bc_ctx_stream": ([vp, C.POINTER(vp)], C.c_int),
        "bc_sync": ([vp], C.c_int),
        "bc_ctx_set_shape": ([vp, C.c_int, C.c_int, C.c_int], C.c_int),
        "bc_pileup_plan": ([C.POINTER(BcReads), i64, C.c_int, C.c_int, C.POINTER(BcPlan)], C.c_int),
        "bc_ctx_set_instance": ([vp, C.c_int], C.c_int),
        "bc_ops_plan": ([C.POINTER(BcReads), i64, C.c_int, C.c_int, C.POINTER(BcOpsPlan)], C.c_int),
        "bc_ctx_set_ops_passes": ([vp, C.c_int], C.c_int),
        "bc_pileup_launch_info": ([C.POINTER(BcReads), i64, C.c_int, C.c_int, C.c_int, u32, C.c_int,
                                   C.POINTER(BcLaunchInfo)], C.c_int),
        "bc_malloc": ([vp, C.c_size_t, C.POINTER(vp)], C.c_int),
        "bc_free": ([vp, vp], C.c_int),
        "bc_memcpy_h2d": ([vp, vp, vp, C.c_size_t], C.c_int),
        "bc_memcpy_d2h": ([vp, vp, vp, C.c_size_t], C.c_int),
        "bc_memset": ([vp, vp, C.c_int, C.c_size_t], C.c_int),
        "bc_reads_upload": ([vp, C.POINTER(BcReads), C.POINTER(BcReads)], C.c_int),
        "bc_reads_free": ([vp, C.POINTER(BcReads)], C.c_int),
        "bc_reads_index_bytes": ([vp, C.POINTER(BcReads), i64, C.c_int, C.POINTER(C.c_size_t)], C.c_int),
        "bc_reads_index": ([vp, C.POINTER(BcReads), i64, C.c_int, vp, C.c_size_t], C.c_int),
        "bc_reads_sort_bytes": ([vp, C.POINTER(BcReads), C.POINTER(C.c_size_t)], C.c_int),
        "bc_reads_sort": ([vp, C.POINTER(BcReads), C.POINTER(BcReads), vp, C.c_size_t], C.c_int),
        "bc_reads_sort_check": ([vp, C.POINTER(BcReads), vp], C.c_int),
        "bc_count": ([vp, C.POINTER(BcReads), i64, u32, C.c_int, vp], C.c_int),
        "bc_range_error": ([vp, C.POINTER(i64)], C.c_int),
        "bc_stats": ([vp, vp, i64, C.c_int, dbl, dbl, vp, vp, vp, vp], C.c_int),
        "bc_summary_work_bytes": ([i64], C.c_size_t),
        "bc_seq_event_bytes": ([i64], C.c_size_t),
        "bc_seq_to_event": ([vp, vp, i64, vp], C.c_int),
        "bc_summary": ([vp, vp, vp, i64, vp, vp], C.c_int),
        "bc_amplicons": ([vp, vp, vp, vp, i64, vp, vp, C.c_int32, vp], C.c_int),
        "bc_pileup_summary_amplicons": ([vp, C.POINTER(BcReads), i64, u32, C.c_int, dbl, dbl, vp, vp, vp, vp, vp, vp,
                                         vp, vp, C.c_int32, vp], C.c_int),
        "bc_bcount_host": ([C.c_int, i64, u32, C.POINTER(BcReads), vp, C.POINTER(i64),
                            C.POINTER(i64)], C.c_int),
        "bc_pileup": ([vp, C.POINTER(BcReads), i64, u32, C.c_int, dbl, dbl, vp, vp, vp, vp, vp],
                      C.c_int),
        "bc_pileup_summary": ([vp, C.POINTER(BcReads), i64, u32, C.c_int, dbl, dbl, vp, vp, vp, vp, vp,
                               vp, vp], C.c_int),
        "bc_pileup_partials": ([vp, C.POINTER(BcReads), i64, u32, C.c_int, dbl, dbl, vp, vp, vp, vp, vp,
                                vp], C.c_int),
        "bc_summary_fold": ([vp, C.c_int, vp, vp, vp], C.c_int),
        "bc_segments_layout": ([vp, C.c_int, vp], C.c_int),
        "bc_pileup_segments": ([vp, C.POINTER(BcReads), C.c_int, vp, vp, vp, i64, vp, u32, C.c_int, dbl, dbl,
                                vp, vp, vp, vp, vp, vp], C.c_int),
        "bc_segments_rebase": ([vp, i64, C.c_int, vp, vp, vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp], C.c_int),
        "bc_amplicons_segments": ([vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int32, vp], C.c_int),
        "bc_graph_begin": ([vp], C.c_int),
        "bc_graph_end": ([vp, C.POINTER(vp)], C.c_int),
        "bc_graph_launch": ([vp, vp], C.c_int),
        "bc_graph_destroy": ([vp], C.c_int),
        "bc_timing_enable": ([vp, C.c_int], C.c_int),
        "bc_timing_report": ([vp, vp, vp], C.c_int),
        "bc_event_record": ([vp, C.c_int], C.c_int),
        "bc_ctx_wait": ([vp, vp], C.c_int),
        "bc_event_elapsed_ms": ([vp, C.c_int, C.c_int, C.POINTER(C.c_float)], C.c_int),
        # BGZF inflate on the device (bc_inflate.hip)
        "bc_bgzf_inflate": ([vp, vp, C.c_uint64, vp, i64, vp, C.c_uint64, vp], C.c_int),
        "bc_bgzf_inflate_host": ([vp, vp, C.c_uint64, vp, i64, vp, C.c_uint64, vp], C.c_int),
        "bc_bgzf_inflate_host_times": ([vp, C.POINTER(dbl * 3), C.POINTER(i64)], C.c_int),
        # BAM record decode on the device (bc_bam.hip)
        "bc_bam_index_bytes": ([C.c_uint64, u32, C.POINTER(C.c_size_t)], C.c_int),
        "bc_bam_index": ([vp, vp, C.c_uint64, C.c_uint64, i64, C.c_int, C.c_int32, u32, vp, C.c_size_t,
                          C.POINTER(BcBamBatch)], C.c_int),
        "bc_bam_fill": ([vp, vp, vp, C.POINTER(BcBamBatch), C.POINTER(BcBamArrays), C.c_int], C.c_int),
        "bc_bam_decoder_create": ([vp, C.c_int, u32, C.POINTER(vp)], C.c_int),
        "bc_bam_decoder_destroy": ([vp], C.c_int),
        "bc_bam_batch_arrays": ([vp, C.POINTER(BcBamArrays)], C.c_int),
        "bc_bam_decoder_stats": ([vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(dbl * 7)], C.c_int),
        "bc_bam_decoder_drop": ([vp], C.c_int),
        # read selection on the device (bc_select.hip)
        "bc_bam_select_bytes": ([i64, i64, C.POINTER(C.c_size_t)], C.c_int),
        "bc_bam_select": ([vp, C.POINTER(BcBamArrays), i64, i64, vp, vp, C.c_int32, vp, C.c_size_t,
                           C.POINTER(BcSelArrays)], C.c_int),
        # row formatting on the device (bc_fmt.hip)
        "bc_fmt_rows_bytes": ([i64, i64, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "bc_fmt_rows": ([vp, C.POINTER(BcFmtArgs), vp, C.c_size_t, vp, vp, i64], C.c_int),
        # BGZF deflate on the device (bc_deflate.hip)
        "bc_bgzf_deflate_bytes": ([i64, i64, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)], C.c_int),
        "bc_bgzf_deflate": ([vp, vp, i64, vp, i64, vp, vp, C.c_size_t, vp, vp, i64], C.c_int),
        "bc_bgzf_deflate_host": ([vp, vp, i64, vp, i64, vp, C.POINTER(i64), C.c_int], C.c_int),
        # multi-GPU (bc_comm.hip)
        "bc_comm_unique_id": ([vp], C.c_int),
        "bc_comm_init": ([vp, vp, C.c_int, C.c_int, C.POINTER(vp)], C.c_int),
        "bc_comm_destroy": ([vp], C.c_int),
        "bc_comm_rank": ([vp, C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int),
        "bc_comm_barrier": ([vp], C.c_int),
        "bc_allgather_i64": ([vp, vp, i64, vp], C.c_int),
        "bc_broadcast_bytes": ([vp, vp, i64, C.c_int], C.c_int),
        "bc_gather_layout": ([vp, C.c_int, vp], C.c_int),
        "bc_gather_bytes": ([vp, vp, i64, vp, vp, C.c_int], C.c_int),
        "bc_gather_dev": ([vp, vp, i64, vp, vp, C.c_int], C.c_int),
        "bc_reduce_i32_dev": ([vp, vp, vp, i64, C.c_int], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise BcError(rc, lib().bc_last_error().decode(errors="replace"))


def build_info() -> str:
    """bc_build_info(): e.g. "gfx950 diag=0 phase_trace=0"."""
    return lib().bc_build_info().decode()


def device_count() -> int:
    n = C.c_int(0)
    check(lib().bc_device_count(C.byref(n)))
    return n.value


def pileup_plan(reads, L: int, shape: str = "auto", tile_waves: int = 0) -> dict:
    """bc_pileup_plan: what bc_pileup would launch for a sorted batch on a reference of L
    positions under (shape, tile_waves).  ``reads``: a DeviceReads, a BcReads, or a dict with
    n_reads, max_span and max_end (only the header is read, never a pointer).  Returns kernel
    ("rc", "solo" or "tiles"), waves_per_tile, block_threads, lds_bytes, blocks, reads_per_tile,
    blocks_per_cu (the workgroups resident per CU; -1 without a device) and tiles_per_wave (the
    sparse sweep's run of tiles per wave in bc_pileup; the fused-summary calls round it up to a
    multiple of 32; 0 for the other kernels)."""
    if isinstance(reads, dict):
        r = BcReads()
        r.n_reads, r.max_span, r.max_end = int(reads["n_reads"]), int(reads["max_span"]), int(reads["max_end"])
        r.sorted, r.seq_layout = 1, BC_SEQ_EVENT
    else:
        r = reads.r if isinstance(reads, DeviceReads) else reads
    p = BcPlan()
    check(lib().bc_pileup_plan(C.byref(r), int(L), SHAPES[shape], int(tile_waves), C.byref(p)))
    return {"kernel": PLAN_KERNELS[p.kernel], "waves_per_tile": p.waves_per_tile, "block_threads": p.block_threads,
            "lds_bytes": p.lds_bytes, "blocks": p.blocks, "blocks_per_cu": p.blocks_per_cu,
            "tiles_per_wave": p.tiles_per_wave, "reads_per_tile": p.reads_per_tile}


def ops_plan(reads, L: int, reads_per_block: int = 0, passes: int = 0) -> dict:
    """bc_ops_plan: what the "ops" shape launches for a batch on a reference of L positions.
    ``reads``: a DeviceReads, a BcReads, or a dict with n_reads, sorted, max_span, max_end and
    seq_bytes (only the header is read, never a pointer).  reads_per_block 0 = from the batch, else
    forced (at most 32768); passes 0 = from the batch, 1 = the single window, 2..OPS_PASSES_MAX =
    that many window passes at most.  Returns reads_per_block, window (4096 positions; 0 for an
    unsorted batch, which has none), passes_max (1: the single-pass kernel; more: a workgroup runs
    up to that many passes over consecutive windows from its first read's start and ends when none
    of its reads reaches further) and blocks.  A sorted batch whose typical read, min(2 x seq_bytes
    / n_reads, max_span), is at most 2048 positions gets passes_max 1 unless passes forces more;
    longer reads get the reads that start within one window per block (at least 4) and the passes
    they can reach."""
    if isinstance(reads, dict):
        r = BcReads()
        r.n_reads, r.sorted = int(reads["n_reads"]), int(reads.get("sorted", 1))
        r.max_span, r.max_end, r.seq_bytes = int(reads["max_span"]), int(reads["max_end"]), int(reads["seq_bytes"])
        r.seq_layout = BC_SEQ_EVENT
    else:
        r = reads.r if isinstance(reads, DeviceReads) else reads
    p = BcOpsPlan()
    check(lib().bc_ops_plan(C.byref(r), int(L), int(reads_per_block), int(passes), C.byref(p)))
    return {"reads_per_block": p.reads_per_block, "window": p.window, "passes_max": p.passes_max, "blocks": p.blocks}


def pileup_launch_info(reads, L: int, shape: str = "auto", tile_waves: int = 0, instance: str = "auto",
                       mbq: int = 0, k: int = 5) -> dict:
    """bc_pileup_launch_info: the instance a bc_pileup call launches on a context set to (shape,
    tile_waves, instance).  ``reads`` as for pileup_plan; a dict may also give n_cigar_words (the
    routing bound's input; default: one op per read).  Returns kernel, lean (bool), waves_per_tile,
    block_threads, lds_bytes, blocks and blocks_per_cu of that very kernel (-1 without a device),
    and ``slice``: the lean walk's slice instance, which the library reports as lean = 1 with
    BC_SLICE_LDS_BYTES of LDS (slice_lds_bytes)."""
    if isinstance(reads, dict):
        r = BcReads()
        r.n_reads, r.max_span, r.max_end = int(reads["n_reads"]), int(reads["max_span"]), int(reads["max_end"])
        r.n_cigar_words = int(reads.get("n_cigar_words", r.n_reads))
        r.sorted, r.seq_layout = 1, BC_SEQ_EVENT
    else:
        r = reads.r if isinstance(reads, DeviceReads) else reads
    p = BcLaunchInfo()
    check(lib().bc_pileup_launch_info(C.byref(r), int(L), SHAPES[shape], int(tile_waves), INSTANCES[instance], int(mbq),
                                      int(k), C.byref(p)))
    is_slice = bool(p.lean) and p.lds_bytes == slice_lds_bytes(p.block_threads // 64, p.waves_per_tile)
    return {"kernel": PLAN_KERNELS[p.kernel], "lean": bool(p.lean), "waves_per_tile": p.waves_per_tile,
            "block_threads": p.block_threads, "lds_bytes": p.lds_bytes, "blocks": p.blocks,
            "blocks_per_cu": p.blocks_per_cu, "slice": is_slice}


def slice_lds_bytes(waves: int, waves_per_tile: int) -> int:
    """BC_SLICE_LDS_BYTES (basecount_hip.h): LDS per workgroup of k_pileup's slice instance."""
    return waves * (1024 + 4096 + 32) + (waves // waves_per_tile) * 1536 + 2048 + 64


class DeviceBuffer:
    """Library-owned HBM allocation."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().bc_malloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            check(lib().bc_free(self.ctx.h, self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, arr: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        check(lib().bc_memcpy_h2d(self.ctx.h, self.ptr, a.ctypes.data, a.nbytes))
        self.ctx._keep.append(a)  # keep host staging alive until the next sync
        return self

    def download(self, dtype, count: int, offset_bytes: int = 0) -> np.ndarray:
        out = np.empty(int(count), dtype)
        if out.nbytes:
            check(lib().bc_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset_bytes,
                                      out.nbytes))
            self.ctx.sync()
        return out

    def zero(self, nbytes: int | None = None):
        check(lib().bc_memset(self.ctx.h, self.ptr, 0, self.nbytes if nbytes is None else nbytes))


def host_reads(b: dict) -> tuple:
    """bc_reads over host numpy arrays (keeps the arrays referenced in the returned tuple)."""
    keep = {}
    for k, dt in (("pos", np.int32), ("cig_beg", np.uint32), ("cig_n", np.uint32),
                  ("seq_nib", np.uint32), ("cigar", np.uint32), ("seq", np.uint8)):
        keep[k] = np.ascontiguousarray(b[k], dt)
    q = b.get("qual")
    keep["qual"] = None if q is None else np.ascontiguousarray(q, np.uint8)
    r = BcReads()
    r.n_reads = keep["pos"].size
    for k in ("pos", "cig_beg", "cig_n", "seq_nib", "cigar", "seq"):
        setattr(r, k, keep[k].ctypes.data if keep[k].size else None)
    r.n_cigar_words = keep["cigar"].size
    r.seq_bytes = keep["seq"].size
    if keep["qual"] is not None:
        r.qual = keep["qual"].ctypes.data if keep["qual"].size else None
        r.qual_bytes = keep["qual"].size
    r.sorted = int(b.get("sorted", 0))
    r.max_span = int(b.get("max_span", 0))
    if b.get("seq_event") is not None:
        # the host already holds the kernels' layout (bcio decoder / bam.seq_to_event): sent as
        # is, no device conversion pass
        keep["seq"] = np.ascontiguousarray(b["seq_event"], np.uint8)
        r.seq = keep["seq"].ctypes.data
        r.seq_layout = BC_SEQ_EVENT
    return r, keep


class DeviceReads:
    """A read batch resident in HBM (library-owned copy of a host batch)."""

    def __init__(self, ctx: "Context", b: dict):
        self.ctx = ctx
        hr, keep = host_reads(b)
        self.r = BcReads()
        check(lib().bc_reads_upload(ctx.h, C.byref(hr), C.byref(self.r)))
        self.n = int(self.r.n_reads)

    def free(self):
        if getattr(self, "r", None) is not None and self.ctx.h:
            check(lib().bc_reads_free(self.ctx.h, C.byref(self.r)))
            self.r = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    def __init__(self, device: int = 0, stream: int | None = None):
        self.device = int(device)
        h = C.c_void_p()
        check(lib().bc_ctx_create(self.device, stream, C.byref(h)))
        self.h = h.value
        self._keep = []
        self.shape_args = ("auto", 0, 0)  # set_shape's arguments in force

    def close(self):
        if self.h:
            lib().bc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def release_scratch(self) -> None:
        """bc_ctx_release_scratch: the context's own grow-only device scratch given back."""
        check(lib().bc_ctx_release_scratch(self.h))

    def set_shape(self, shape: str = "auto", tile_waves: int = 0, reads_per_block: int = 0) -> None:
        """Kernel-shape override for bc_count / bc_pileup (bc_ctx_set_shape): "auto", "tile",
        "rc", "tile_no_solo" or "ops" (the scan-expanded k_ops for batches of many-op reads, never
        chosen by "auto"; bc_count under it also takes unsorted batches); tile_waves 0/1/2/4/8;
        reads_per_block 0 or 1..32768.  ``shape_args`` keeps the arguments in force."""
        check(lib().bc_ctx_set_shape(self.h, SHAPES[shape], int(tile_waves), int(reads_per_block)))
        self.shape_args = (shape, int(tile_waves), int(reads_per_block))

    def set_instance(self, instance: str = "auto") -> None:
        """The tiled k_pileup's instance (bc_ctx_set_instance): "auto" (the lean walk while the
        batch's bound on multi-run reads is small, over per-read slices when reads can be longer
        than a tile), "general", "lean" or "slice" (A/B runs and tests; all are exact on every
        batch)."""
        check(lib().bc_ctx_set_instance(self.h, INSTANCES[instance]))

    def set_ops_passes(self, passes: int = 0) -> None:
        """The window passes of the "ops" shape's kernel (bc_ctx_set_ops_passes): 0 (ops_plan
        decides from the batch), 1 (the single window and its launch) or 2..OPS_PASSES_MAX (that
        many at most, on any sorted batch).  A/B runs and tests; every setting counts the same."""
        check(lib().bc_ctx_set_ops_passes(self.h, int(passes)))

    def sync(self):
        check(lib().bc_sync(self.h))
        self._keep.clear()

    def stream(self) -> int:
        s = C.c_void_p()
        check(lib().bc_ctx_stream(self.h, C.byref(s)))
        return s.value or 0

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    # kernels ---------------------------------------------------------------------------
    def count(self, reads, ref_len: int, mbq: int, ncols: int, d_hist: int) -> None:
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_count(self.h, C.byref(r), int(ref_len), int(mbq), int(ncols), d_hist))

    def index_bytes(self, reads, L: int, what: int = BC_INDEX_AUTO) -> int:
        """bc_reads_index_bytes: device bytes the batch's index needs (0: nothing to build)."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        n = C.c_size_t(0)
        check(lib().bc_reads_index_bytes(self.h, C.byref(r), int(L), int(what), C.byref(n)))
        return int(n.value)

    def index(self, reads, L: int, d_mem, nbytes: int, what: int = BC_INDEX_AUTO) -> None:
        """bc_reads_index: build the batch's device index (run records / chunk summaries / tile
        index) into d_mem on the stream and set the index fields of the bc_reads in place."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_reads_index(self.h, C.byref(r), int(L), int(what), d_mem, int(nbytes)))

    def sort_bytes(self, reads) -> int:
        """bc_reads_sort_bytes: device bytes the sorted copy of an unsorted batch needs."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        n = C.c_size_t(0)
        check(lib().bc_reads_sort_bytes(self.h, C.byref(r), C.byref(n)))
        return int(n.value)

    def sort(self, reads, d_mem, nbytes: int, check_flags: bool = True) -> BcReads:
        """bc_reads_sort: a coordinate-sorted copy of the batch, built on the device into d_mem
        (stream-ordered: the call only enqueues); returns its bc_reads (no index yet).  With
        ``check_flags`` the device's error flags are read at once (sort_check, a sync); without it the
        caller runs sort_check(reads, d_mem) later, e.g. after the batch's kernels."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        out = BcReads()
        check(lib().bc_reads_sort(self.h, C.byref(r), C.byref(out), d_mem, int(nbytes)))
        if check_flags:
            self.sort_check(r, d_mem)
        return out

    def sort_check(self, reads, d_mem) -> None:
        """bc_reads_sort_check: waits for the stream, raises BcError (BC_E_ARG) if the sort of
        ``reads`` into d_mem saw a start outside [0, max_end] or overlapping sequences."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_reads_sort_check(self.h, C.byref(r), d_mem))

    def pileup(self, reads, L, mbq, k, nf, nf2, d_counts, d_cov, d_pc, d_ent, d_sec):
        """Fused kernel 1 + kernel 2 (bc_pileup) for a coordinate-sorted batch: one launch."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_pileup(self.h, C.byref(r), int(L), int(mbq), int(k), float(nf), float(nf2),
                              d_counts, d_cov, d_pc, d_ent, d_sec))

    def pileup_summary(self, reads, L, mbq, k, nf, nf2, d_counts, d_cov, d_pc, d_ent, d_sec, d_work,
                       d_out):
        """bc_pileup + bc_summary in one call (the sparse sweep computes the summary partials)."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_pileup_summary(self.h, C.byref(r), int(L), int(mbq), int(k), float(nf),
                                      float(nf2), d_counts, d_cov, d_pc, d_ent, d_sec, d_work, d_out))

    def pileup_partials(self, reads, L, mbq, k, nf, nf2, d_counts, d_cov, d_pc, d_ent, d_sec, d_work):
        """bc_pileup_partials: pileup + the summary's per-buffer partials (fold them with
        summary_fold)."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_pileup_partials(self.h, C.byref(r), int(L), int(mbq), int(k), float(nf),
                                       float(nf2), d_counts, d_cov, d_pc, d_ent, d_sec, d_work))

    def summary_fold(self, lens, works, outs) -> None:
        """bc_summary_fold over several references (device pointers works / outs)."""
        n = len(lens)
        la = (C.c_int64 * max(1, n))(*[int(x) for x in lens])
        wa = (C.c_void_p * max(1, n))(*works)
        oa = (C.c_void_p * max(1, n))(*outs)
        check(lib().bc_summary_fold(self.h, n, la, wa, oa))

    def pileup_segments(self, reads, n_seg, d_ref_len, d_read_beg, d_voff, virt_len, d_vpos, mbq, k, nf, nf2,
                        d_counts, d_cov, d_pc, d_ent, d_sec, d_sum=None) -> None:
        """bc_pileup_segments: n_seg references as one virtual reference of virt_len positions
        (segments_layout), one pileup launch; ``reads`` carries the original starts, the device
        table (d_ref_len, d_read_beg, d_voff: int64) says which reads are whose.  d_sum: [n_seg][4]
        doubles (bc_summary per segment) or None."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_pileup_segments(self.h, C.byref(r), int(n_seg), d_ref_len, d_read_beg, d_voff,
                                       int(virt_len), d_vpos, int(mbq), int(k), float(nf), float(nf2),
                                       d_counts, d_cov, d_pc, d_ent, d_sec, d_sum))

    # BGZF inflate -------------------------------------------------------------------------
    def bgzf_inflate(self, d_comp: int, comp_bytes: int, d_blocks: int, n: int, d_out: int, out_bytes: int,
                     d_status: int) -> None:
        """bc_bgzf_inflate: k_inflate over n device-resident bc_zblock descriptors (ZBLOCK_DTYPE),
        stream-ordered; one status byte per block (0 = inflated)."""
        check(lib().bc_bgzf_inflate(self.h, d_comp, int(comp_bytes), d_blocks, int(n), d_out, int(out_bytes),
                                    d_status))

    def bgzf_inflate_host(self, comp: np.ndarray, blocks: np.ndarray, out: np.ndarray) -> np.ndarray:
        """bc_bgzf_inflate_host over host arrays (uint8 comp / out, ZBLOCK_DTYPE blocks): blocking;
        returns the status bytes."""
        assert comp.dtype == np.uint8 and out.dtype == np.uint8 and blocks.dtype == ZBLOCK_DTYPE
        comp, blocks = np.ascontiguousarray(comp), np.ascontiguousarray(blocks)
        assert out.flags.c_contiguous and out.flags.writeable
        status = np.empty(max(1, blocks.size), np.uint8)
        check(lib().bc_bgzf_inflate_host(self.h, comp.ctypes.data, comp.size, blocks.ctypes.data, blocks.size,
                                         out.ctypes.data, out.size, status.ctypes.data))
        return status[:blocks.size]

    def bgzf_inflate_times(self) -> dict:
        """Cumulative device time of this context's bgzf_inflate_host calls (ms) and their blocks."""
        ms, nb = (C.c_double * 3)(), C.c_int64(0)
        check(lib().bc_bgzf_inflate_host_times(self.h, C.byref(ms), C.byref(nb)))
        return {"upload_ms": ms[0], "kernel_ms": ms[1], "download_ms": ms[2], "blocks": nb.value}

    def inflater(self) -> tuple:
        """(function address, context handle) for bcio_stream_set_inflater: the library's own
        bc_bgzf_inflate_host, so no Python runs on the stream's fill path."""
        return C.cast(lib().bc_bgzf_inflate_host, C.c_void_p).value, self.h

    # BAM record decode on the device (bc_bam.hip) --------------------------------------------
    def bam_index(self, d_raw: int, raw_bytes: int, first: int, max_records: int, final: bool, n_refs: int,
                  d_work: int, work_bytes: int, seg_bytes: int = 0) -> BcBamBatch:
        """bc_bam_index: the record chain of d_raw[first, raw_bytes) into d_work (blocking: it
        returns the counts that size the arrays).  A non-zero ``status`` declines the fill."""
        b = BcBamBatch()
        check(lib().bc_bam_index(self.h, d_raw, int(raw_bytes), int(first), int(max_records), int(bool(final)),
                                 int(n_refs), int(seg_bytes), d_work, int(work_bytes), C.byref(b)))
        return b

    def bam_fill(self, d_raw: int, d_work: int, batch: BcBamBatch, arrays: BcBamArrays, want_qual: bool) -> None:
        """bc_bam_fill: the indexed batch's arrays, stream-ordered (capturable, no allocation)."""
        check(lib().bc_bam_fill(self.h, d_raw, d_work, C.byref(batch), C.byref(arrays), int(bool(want_qual))))

    def bam_decode(self, d_raw: int, raw_bytes: int, first: int, max_records: int, final: bool, n_refs: int,
                   want_qual: bool = True, seg_bytes: int = 0):
        """Index and fill one batch into fresh device buffers: a DeviceBamBatch, or None with the
        declining BcBamBatch when the device declines the fill ((batch, None): decode it on the
        host).  ``max_records`` < 0: no limit."""
        work = self.alloc(bam_index_bytes(raw_bytes, seg_bytes))
        lim = (1 << 63) - 1 if max_records < 0 else int(max_records)
        b = self.bam_index(d_raw, raw_bytes, first, lim, final, n_refs, work.ptr, work.nbytes, seg_bytes)
        if b.status != 0:
            work.free()
            return b, None
        out = DeviceBamBatch(self, b, want_qual)
        self.bam_fill(d_raw, work.ptr, b, out.arrays, want_qual)
        self.sync()  # the work buffer is released here; the arrays are complete
        work.free()
        return b, out

    def bam_select(self, rec: BcBamArrays, n: int, min_mapq: int, d_ref_sel: int, d_ref_len: int, n_refs: int,
                   d_work: int, work_bytes: int, out: BcSelArrays) -> None:
        """bc_bam_select: bcio_select on a decoded batch's device arrays, stream-ordered (capturable,
        no allocation).  The header's status says whether the outputs are to be used."""
        mmq = max(min(int(min_mapq), 1 << 40), -(1 << 40))
        check(lib().bc_bam_select(self.h, C.byref(rec), int(n), mmq, d_ref_sel, d_ref_len, int(n_refs), d_work,
                                  int(work_bytes), C.byref(out)))

    def bgzf_deflate(self, d_text: int, text_cap: int, d_span_off: int, n_spans: int, d_gate, d_work: int,
                     work_bytes: int, d_out_small: int, d_comp: int, comp_cap: int) -> None:
        """bc_bgzf_deflate: spans of device text into BGZF blocks in d_comp, stream-ordered (capturable,
        no allocation).  d_out_small: the 64-byte header (DFL_HEADER_DTYPE) and span_coff[n_spans + 1];
        d_gate: None or a device int32 that, non-zero, turns the call into a header write (DFL_GATED)."""
        check(lib().bc_bgzf_deflate(self.h, d_text, int(text_cap), d_span_off, int(n_spans), d_gate, d_work,
                                    int(work_bytes), d_out_small, d_comp, int(comp_cap)))

    def fmt_rows(self, args: BcFmtArgs, d_work: int, work_bytes: int, d_out: int, d_text: int, text_cap: int) -> None:
        """bc_fmt_rows: the TSV rows of device-resident outputs into d_text, stream-ordered (capturable,
        no allocation).  d_out: the 64-byte header (FMT_HEADER_DTYPE) and seg_off[n_seg + 1]; the
        header's status says whether the text is to be used."""
        check(lib().bc_fmt_rows(self.h, C.byref(args), d_work, int(work_bytes), d_out, d_text, int(text_cap)))

    def capture(self, fn) -> "Graph":
        """Record the compute calls made by fn() into a hipGraph (replay with Graph.launch)."""
        check(lib().bc_graph_begin(self.h))
        try:
            fn()
        finally:
            g = C.c_void_p()
            rc = lib().bc_graph_end(self.h, C.byref(g))
        check(rc)
        return Graph(self, g.value)

    def timing(self, on: bool = True) -> None:
        check(lib().bc_timing_enable(self.h, int(bool(on))))

    def timing_report(self) -> dict:
        """{kernel: (launches, mean_us)} since the last report (synchronises)."""
        n = np.zeros(KERNEL_IDS, np.int64)
        us = np.zeros(KERNEL_IDS, np.float64)
        check(lib().bc_timing_report(self.h, n.ctypes.data, us.ctypes.data))
        return {name: (int(n[i]), float(us[i])) for i, name in enumerate(KERNEL_NAMES) if n[i]}

    def seq_to_event(self, d_bam: int, seq_bytes: int, d_event: int) -> None:
        """BAM-packed sequence -> BC_SEQ_EVENT (d_event may alias d_bam; it needs
        seq_event_bytes(seq_bytes) bytes)."""
        check(lib().bc_seq_to_event(self.h, d_bam, int(seq_bytes), d_event))

    def wait(self, other: "Context") -> None:
        """bc_ctx_wait: this context's later work waits for everything enqueued on `other`."""
        check(lib().bc_ctx_wait(self.h, other.h))

    def event_record(self, slot: int) -> None:
        """Record hipEvent `slot` on the context's stream (region timing)."""
        check(lib().bc_event_record(self.h, int(slot)))

    def event_elapsed_ms(self, slot0: int, slot1: int) -> float:
        ms = C.c_float(0.0)
        check(lib().bc_event_elapsed_ms(self.h, int(slot0), int(slot1), C.byref(ms)))
        return float(ms.value)

    def range_error(self) -> int:
        v = C.c_int64(-1)
        check(lib().bc_range_error(self.h, C.byref(v)))
        return v.value

    def stats(self, d_hist, L, k, nf, nf2, d_cov, d_pc, d_ent, d_sec) -> None:
        check(lib().bc_stats(self.h, d_hist, int(L), int(k), float(nf), float(nf2), d_cov, d_pc,
                             d_ent, d_sec))

    def summary(self, d_cov, d_ent, L, d_work, d_out) -> None:
        check(lib().bc_summary(self.h, d_cov, d_ent, int(L), d_work, d_out))

    def pileup_summary_amplicons(self, reads, L, mbq, k, nf, nf2, d_counts, d_cov, d_ent, d_sec, d_work, d_out,
                                 d_lo, d_hi, n_tiles, d_amp) -> None:
        """bc_pileup_summary_amplicons: --summarise-with-bed for one reference (the summary's 4
        doubles into d_out, 6 per amplicon window into d_amp); a deep batch's tail after kernel 1
        is kernel 2 + ONE launch."""
        r = reads.r if isinstance(reads, DeviceReads) else reads
        check(lib().bc_pileup_summary_amplicons(self.h, C.byref(r), int(L), int(mbq), int(k), float(nf), float(nf2),
                                                d_counts, d_cov, d_ent, d_sec, d_work, d_out, d_lo, d_hi,
                                                int(n_tiles), d_amp))

    def amplicons(self, d_cov, d_ent, d_sec, L, d_lo, d_hi, n_tiles, d_out) -> None:
        check(lib().bc_amplicons(self.h, d_cov, d_ent, d_sec, int(L), d_lo, d_hi, int(n_tiles),
                                 d_out))

    def segments_rebase(self, n_reads, n_seg, d_read_beg, d_cig_base, d_nib_base, cig_words_total, nib_total,
                        d_cig_beg, d_seq_nib, d_cig_beg_out=None, d_seq_nib_out=None) -> None:
        """bc_segments_rebase: cig_beg / seq_nib of a cohort batch's reads moved by their file's bases
        (uint64 per segment); in place unless outputs are given."""
        check(lib().bc_segments_rebase(self.h, int(n_reads), int(n_seg), d_read_beg, d_cig_base, d_nib_base,
                                       int(cig_words_total), int(nib_total), d_cig_beg, d_seq_nib,
                                       d_cig_beg if d_cig_beg_out is None else d_cig_beg_out,
                                       d_seq_nib if d_seq_nib_out is None else d_seq_nib_out))

    def amplicons_segments(self, d_cov, d_ent, d_sec, n_seg, d_ref_len, d_voff, d_lo, d_hi, n_tiles, d_out) -> None:
        """bc_amplicons_segments: the windows on every segment's own slice, d_out [n_seg][n_tiles][6]."""
        check(lib().bc_amplicons_segments(self.h, d_cov, d_ent, d_sec, int(n_seg), d_ref_len, d_voff, d_lo, d_hi,
                                          int(n_tiles), d_out))


class Graph:
    def __init__(self, ctx: Context, h: int):
        self.ctx, self.h = ctx, h

    def launch(self):
        check(lib().bc_graph_launch(self.ctx.h, self.h))

    def __del__(self):
        try:
            if self.h:
                lib().bc_graph_destroy(self.h)
                self.h = None
        except Exception:
            pass


class BamDecoder:
    """bc_bam_decoder: a stream's record decoder on this context's GPU (bam.BamStream(device_decode=...)
    hands its four C callbacks to the stream, so no Python runs between a fill and its batches)."""

    def __init__(self, ctx: "Context", want_qual: bool = True, seg_bytes: int = 0):
        self.ctx = ctx
        h = C.c_void_p()
        check(lib().bc_bam_decoder_create(ctx.h, int(bool(want_qual)), int(seg_bytes), C.byref(h)))
        self.h = h.value
        self.want_qual = bool(want_qual)

    def callbacks(self) -> tuple:
        """(user, fill, next, pending, release) addresses for bcio_decoder."""
        L = lib()
        return (self.h,) + tuple(C.cast(getattr(L, "bc_bam_decoder_" + n), C.c_void_p).value
                                 for n in ("fill", "next", "pending", "release"))

    def stats(self) -> dict:
        rep, dec, ms = C.c_int64(0), C.c_int64(0), (C.c_double * 7)()
        check(lib().bc_bam_decoder_stats(self.h, C.byref(rep), C.byref(dec), C.byref(ms)))
        return {"repaired": rep.value, "declined": dec.value, "upload_ms": ms[0], "inflate_ms": ms[1],
                "index_ms": ms[2], "fill_ms": ms[3], "download_ms": ms[4], "fill_wall_ms": ms[5],
                "next_wall_ms": ms[6]}

    def drop(self) -> None:
        """Let the pending bytes go (the stream is closed)."""
        if self.h and self.ctx.h:
            check(lib().bc_bam_decoder_drop(self.h))

    def close(self) -> None:
        if self.h and self.ctx.h:
            lib().bc_bam_decoder_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bam_batch_arrays(handle: int) -> BcBamArrays:
    """The device pointers of a batch a BamDecoder produced (bcio_device_handle's handle)."""
    a = BcBamArrays()
    check(lib().bc_bam_batch_arrays(handle, C.byref(a)))
    return a


def bam_index_bytes(raw_bytes: int, seg_bytes: int = 0) -> int:
    """bc_bam_index_bytes: the work buffer of bc_bam_index (seg_bytes 0: the default, 64 KiB)."""
    n = C.c_size_t(0)
    check(lib().bc_bam_index_bytes(int(raw_bytes), int(seg_bytes), C.byref(n)))
    return int(n.value)


class DeviceBamBatch:
    """The arrays of one device-decoded batch (bcio_records' fields) in HBM; ``download()`` gives
    them as numpy arrays, trimmed to the batch's sizes."""

    def __init__(self, ctx: "Context", batch: BcBamBatch, want_qual: bool = True):
        self.ctx, self.batch, self.want_qual = ctx, batch, bool(want_qual)
        n, cw, sb = int(batch.n), int(batch.cigar_words), int(batch.seq_bytes)
        self.sizes = {name: int(cnt(n, cw, sb)) for name, _, cnt in BAM_ARRAYS}
        self.buffers = {}
        self.arrays = BcBamArrays()
        for name, dt, _ in BAM_ARRAYS:
            if name == "qual" and not want_qual:
                continue
            buf = ctx.alloc(max(16, self.sizes[name] * np.dtype(dt).itemsize))
            self.buffers[name] = buf
            setattr(self.arrays, name, buf.ptr)
        self.arrays.n_cap, self.arrays.cigar_cap, self.arrays.seq_cap = n, cw, sb

    def download(self) -> dict:
        out = {name: self.buffers[name].download(dt, self.sizes[name])
               for name, dt, _ in BAM_ARRAYS if name in self.buffers}
        out["n"] = int(self.batch.n)
        return out

    def free(self) -> None:
        for b in self.buffers.values():
            b.free()
        self.buffers = {}


def seq_event_bytes(seq_bytes: int) -> int:
    return int(lib().bc_seq_event_bytes(int(seq_bytes)))


def summary_work_bytes(L: int) -> int:
    return int(lib().bc_summary_work_bytes(int(L)))


def segments_layout(ref_lens) -> np.ndarray:
    """bc_segments_layout: the virtual offsets int64 [n + 1] of n references placed one after the
    other, each on a 64-position boundary (host arithmetic, no GPU); BcError (BC_E_ARG) for an
    empty list, a length <= 0 or a total past 2^31 - 128."""
    a = np.ascontiguousarray(ref_lens, np.int64)
    out = np.zeros(a.size + 1, np.int64)
    check(lib().bc_segments_layout(a.ctypes.data if a.size else None, int(a.size), out.ctypes.data))
    return out
