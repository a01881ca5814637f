"""BGZF output ("Device deflate").

``Writer`` puts plain bytes (compressed here by ``bc_bgzf_deflate_host``, the host twin of the device
kernels: the same bytes the device writes for the same text) and already compressed runs of whole
blocks (the device's) into one BGZF stream on ``sys.stdout``'s binary layer, and appends the EOF
block on close.  Every ``write`` starts a new block, so what is written in (reference, position)
order stays readable by ``gzip -dc`` and indexable by ``tabix -s1 -b2 -e2 -S1``.
``blocks`` parses a stream back into its blocks.
"""
from __future__ import annotations

import struct

from . import fmt

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 65280  # input bytes of a block
_HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")


def compress(data, nthreads: int = 16):
    """The BGZF blocks of ``data`` (bytes-like), cut every 65,280 bytes; no EOF block.  Empty data
    gives no block."""
    from . import device as D

    if not len(data):
        return b""
    return memoryview(D.bgzf_deflate_host(data, None, nthreads)[0])


def blocks(data) -> list:
    """``(offset, bsize, isize, crc)`` of every block of a BGZF stream (bsize: the whole block's
    bytes); ValueError where the stream is not a sequence of whole blocks with this project's header."""
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 28 or data[at:at + 16] != _HEAD:
            raise ValueError(f"no BGZF block header at byte {at}")
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        if bsize < 28 or at + bsize > len(data):
            raise ValueError(f"block at byte {at} leaves the stream")
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        out.append((at, bsize, isize, crc))
        at += bsize
    return out


class Writer:
    """One BGZF stream on sys.stdout (as ``fmt.write_bytes`` writes: the binary layer when there is
    one).  ``write``: plain bytes; ``write_blocks``: a run of whole blocks; ``close``: the EOF block."""

    def __init__(self, nthreads: int = 16):
        self.nthreads = int(nthreads)
        self.text_bytes = self.comp_bytes = 0
        self.closed = False

    def write(self, data) -> None:
        if len(data):
            self.text_bytes += len(data)
            self.write_blocks(compress(data, self.nthreads))

    def write_blocks(self, run) -> None:
        if len(run):
            self.comp_bytes += len(run)
            fmt.write_bytes(run)

    def close(self) -> None:
        if not self.closed:
            self.closed = True
            self.comp_bytes += len(EOF)
            fmt.write_bytes(EOF)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        return False
