"""BGZF input is read through ``fasta_io`` (``Engine.bgzf_inflate``); this module is the output side and the checkers.

BGZF output (``--bgzip``): the writers' bytes go to one of libmsim's output channels in BGZF mode, which compresses
them on the device (csrc/bgzf.hip) and writes the members (csrc/file_io.hip).  Also a pure-Python reader of the BGZF
structure (SAM/BAM specification section 4.1) and a zlib-made reference file, for checks and measurements."""
from __future__ import annotations

import struct
import zlib

import numpy as np

BGZF_BLOCK = 65280                      # uncompressed bytes per member, as bgzip
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

FASTA_CHANNEL = 0
VCF_CHANNEL = 1


class BgzfError(Exception):
    """The bytes are not a well-formed BGZF file."""


class BgzfSink:
    """A binary file-like object for FastaWriter / VcfWriter: what is written is the uncompressed stream of a BGZF file.

    Host bytes written before an engine is attached (the VCF header: ``Mutator.__init__`` runs before the engine exists)
    are held here and go first.  ``fileno()`` / ``tell()`` name the span the next native transfer appends to (libmsim
    checks that the offset equals the stream's length); ``seek(pos)`` after such a transfer moves the stream's end."""

    HOLD = 4 << 20                      # host bytes gathered before they are handed to the channel

    def __init__(self, fname, channel: int, device: int = 0):
        self._f = open(fname, "w+b")
        self._channel = channel
        self._device = device
        self._eng = None
        self._held: list = []
        self._nheld = 0
        self._pos = 0                   # uncompressed bytes so far (held ones included)
        self.sizes = None               # (compressed, uncompressed) once closed

    @property
    def closed(self) -> bool:
        return self._f.closed

    def attach(self, engine) -> None:
        engine.bgzf_open(self._channel, self._f.fileno())
        self._eng = engine
        self.flush()

    def write(self, data) -> int:
        b = bytes(data)
        if b:
            self._held.append(b)
            self._nheld += len(b)
            self._pos += len(b)
            if self._eng is not None and self._nheld >= self.HOLD:
                self.flush()
        return len(b)

    def flush(self) -> None:
        if self._eng is not None and self._held:
            data = b"".join(self._held)
            self._held, self._nheld = [], 0
            self._eng.bgzf_append(self._channel, data)

    def tell(self) -> int:
        return self._pos

    def seek(self, pos: int) -> None:
        self.flush()
        self._pos = int(pos)

    def fileno(self) -> int:
        return self._f.fileno()

    def close(self) -> None:
        if self._f.closed:
            return
        own = None
        try:
            if self._eng is None:       # (nothing reached the device yet: the held bytes still go through it)
                from . import _ffi
                own = _ffi.Engine(self._device)
                self.attach(own)
            self.flush()
            self.sizes = self._eng.bgzf_close(self._channel)
        finally:
            self._eng = None
            if own is not None:
                own.close()
            self._f.close()


class HostRegion:
    """Stands in for ``MappedRegion`` when the output is a BGZF stream: a host buffer whose bytes are appended to the
    stream by ``close``."""
    __slots__ = ("nbytes", "view")

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        self.view = np.zeros(self.nbytes, dtype=np.uint8)

    def close(self, fileobj):
        if self.nbytes:
            fileobj.write(memoryview(self.view))
        self.view = None


def parse_members(data: bytes):
    """The members of a BGZF file as (offset, bsize, isize, crc32, deflate payload) tuples; raises BgzfError on any
    deviation from the specification (section 4.1: gzip member, FEXTRA with the 'BC' subfield, BSIZE = member size - 1)."""
    out = []
    pos, n = 0, len(data)
    while pos < n:
        if n - pos < 28:
            raise BgzfError(f"truncated member at {pos}")
        id1, id2, cm, flg, _mtime, _xfl, _os, xlen = struct.unpack_from("<BBBBIBBH", data, pos)
        if (id1, id2, cm) != (0x1F, 0x8B, 8) or not flg & 4:
            raise BgzfError(f"not a gzip member with FEXTRA at {pos}")
        x, xend, bsize = pos + 12, pos + 12 + xlen, None
        while x < xend:
            si1, si2, slen = struct.unpack_from("<BBH", data, x)
            if si1 == 66 and si2 == 67 and slen == 2:
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        if bsize is None:
            raise BgzfError(f"no BC subfield at {pos}")
        end = pos + bsize + 1
        if end > n:
            raise BgzfError(f"BSIZE of the member at {pos} runs past the end")
        crc, isize = struct.unpack_from("<II", data, end - 8)
        out.append((pos, bsize, isize, crc, data[xend:end - 8]))
        pos = end
    return out


def inflate_members(data):
    """The decompressed bytes of each member in turn, each checked as ``check_file`` does (for large files)."""
    if bytes(data[-28:]) != EOF_BLOCK:
        raise BgzfError("no EOF marker at the end")
    for pos, bsize, isize, crc, payload in parse_members(data):
        if bsize + 1 > 65536 or isize > BGZF_BLOCK:
            raise BgzfError(f"member at {pos}: {bsize + 1} bytes, ISIZE {isize}")
        d = zlib.decompressobj(-15)
        raw = d.decompress(payload) + d.flush()
        if not d.eof or d.unused_data:
            raise BgzfError(f"member at {pos}: deflate data do not end with the member")
        if len(raw) != isize or zlib.crc32(raw) != crc:
            raise BgzfError(f"member at {pos}: ISIZE / CRC32 mismatch")
        yield raw


def check_file(data: bytes) -> bytes:
    """Checks every member (BGZF framing, ISIZE <= 65 280, inflates on its own, CRC32 and ISIZE match) and the trailing
    EOF marker; returns the decompressed bytes."""
    return b"".join(inflate_members(data))


def make_member(blk: bytes, payload: bytes) -> bytes:
    """One BGZF member around the raw deflate data ``payload`` of ``blk``."""
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
            + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", zlib.crc32(blk), len(blk)))


def zlib_bgzf(data: bytes, level: int = 1, strategy: int = zlib.Z_DEFAULT_STRATEGY, block: int = BGZF_BLOCK) -> bytes:
    """``data`` as BGZF made by Python's zlib at ``level`` (same 65 280-byte blocking): the yardstick for sizes, and with
    ``strategy`` (``zlib.Z_FIXED`` ...) the source of members of every deflate block type for the inflate tests."""
    out = []
    for a in range(0, len(data), block):
        blk = data[a:a + block]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        out.append(make_member(blk, c.compress(blk) + c.flush()))
    out.append(EOF_BLOCK)
    return b"".join(out)
