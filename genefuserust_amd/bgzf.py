"""BGZF-compressed files through the device: libgfinflate.so (include/gf_inflate.h) and the host side that drives it.

A ``.fq.gz`` or ``.fa.gz`` written by a sequencer or by ``bgzip`` is BGZF, a series of independent gzip members of at
most 64 KiB of text.  The streamed routes otherwise inflate such a file with the host's zlib on their upload threads;
with ``inflate="device"`` (or ``"auto"``) the compressed bytes cross the link as they are and are inflated there:

    file  --read, whole members (gf_if_walk_blocks), upload thread-->  pinned staging block of compressed bytes + the
    members' table  --H2D, copy stream-->  the slot's compressed buffer  --gf_if_inflate_device, copy stream-->  the
    slot's text buffer, behind the text the previous chunk's last member left over  -->  the totals read back on the
    upload thread: a failed member raises there.

The text stream and its pieces are those of the host route: a side asks for ``nbytes`` of text and gets exactly that
many, fewer only at the end of the file.  Members do not end where chunks end, so the text of the member that straddles
a chunk's end stays on the device (less than 64 KiB) and comes first in the next chunk.  ``BgzfSource`` — which members
go into which chunk — needs no GPU.  No CPU fallback: without the library and a GPU every device call raises.
"""
from __future__ import annotations

import ctypes as C
import gzip
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib

IF_LIB_PATH = os.path.join(_lib._HERE, "libgfinflate.so")

ROW = 6                     # int64 per table row (GF_IF_ROW_INT64)
MAX_TEXT = 1 << 16          # bytes of text, and of compressed bytes, a BGZF member has at most
WALK_END, WALK_INSIDE, WALK_BUDGET, WALK_CAPACITY, WALK_NOT_BGZF = range(5)
INFLATE_MODES = ("host", "auto", "device")

STATUS_TEXT = {
    1: "reserved block type", 2: "stored block length check", 3: "too many length or distance codes",
    4: "over-subscribed code", 5: "incomplete code", 6: "repeat with no length before it",
    7: "code lengths past their count", 8: "no end-of-block code", 9: "invalid literal/length symbol",
    10: "invalid distance symbol", 11: "distance too far back", 12: "more text than ISIZE", 13: "less text than ISIZE",
    14: "compressed data ended before the end-of-stream marker was reached", 15: "CRC check failed",
    16: "member outside its buffers", 17: "invalid code", 18: "trailing bytes in the member"}

_vp, _i64 = C.c_void_p, C.c_int64
# libgfinflate.so, loaded (once) after libgfmatch.so
lib, check = _lib.companion(IF_LIB_PATH, "device inflate", "gf_if_last_error", {
    "gf_if_walk_blocks": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "gf_if_workspace_bytes": (_i64, [_i64]),
    "gf_if_inflate_device": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "gf_if_copy_from_host_device": (C.c_int, [_vp, _vp, _i64, _vp]),
    "gf_if_last_error": (C.c_char_p, []),
})


class Walk(NamedTuple):
    """What ``walk_blocks`` found: the table rows of ``members`` whole members, which take the first ``comp_bytes`` of
    the range and hold ``text_bytes`` of text; ``why`` the walk stopped (``WALK_*``) at offset ``stop``."""
    table: np.ndarray
    members: int
    comp_bytes: int
    text_bytes: int
    why: int
    stop: int


def walk_blocks(comp, file_offset: int = 0, text_budget: int = 1 << 62, max_members: Optional[int] = None,
                table: Optional[np.ndarray] = None) -> Walk:
    """``gf_if_walk_blocks`` over ``comp`` (bytes, or a C-contiguous uint8 array): host code, no GPU."""
    a = np.frombuffer(comp, dtype=np.uint8) if not isinstance(comp, np.ndarray) else comp
    assert a.dtype == np.uint8 and a.ndim == 1 and a.flags.c_contiguous
    if table is None:
        # (a member takes at least 28 bytes)
        table = np.empty((a.size // 28 + 1 if max_members is None else max_members, ROW), dtype=np.int64)
    cap = table.shape[0] if max_members is None else min(int(max_members), table.shape[0])
    res = np.zeros(5, dtype=np.int64)
    check(lib().gf_if_walk_blocks(a.ctypes.data if a.size else None, a.size, int(file_offset), int(text_budget), cap,
                                  table.ctypes.data if table.size else None, res.ctypes.data))
    n = int(res[0])
    return Walk(table[:n], n, int(res[1]), int(res[2]), int(res[3]), int(res[4]))


def inflate_device(comp, table, out, stream=None):
    """``gf_if_inflate_device``, asynchronously: the members of ``table`` (int64 device tensor [n, 6]) from ``comp`` into
    ``out`` (uint8 device tensors).  Returns (statuses int32[n], totals int64[4]), device tensors."""
    import torch
    _lib.need_device_tensors("inflate_device", comp, table, out)
    assert comp.dtype == torch.uint8 and out.dtype == torch.uint8 and table.dtype == torch.int64
    assert comp.is_contiguous() and out.is_contiguous() and table.is_contiguous()
    dev = table.device
    n = table.numel() // ROW
    status = _lib.for_stream(torch.empty(max(n, 1), dtype=torch.int32, device=dev), stream)
    totals = _lib.for_stream(torch.empty(4, dtype=torch.int64, device=dev), stream)
    check(lib().gf_if_inflate_device(comp.data_ptr() if comp.numel() else None, comp.numel(),
                                     table.data_ptr() if n else None, n, out.data_ptr() if out.numel() else None,
                                     out.numel(), status.data_ptr(), totals.data_ptr(), None, 0,
                                     _lib.stream_handle(dev, stream)))
    return status[:n], totals


def is_bgzf(path: str) -> bool:
    """Whether the file's first member is BGZF (an empty file is not)."""
    with open(path, "rb") as f:
        head = f.read(MAX_TEXT)
    w = walk_blocks(head, max_members=1)
    return w.members == 1


def use_device_inflate(path: str, inflate: str) -> bool:
    """What ``inflate`` means for this file: True when its compressed bytes go to the device.  ``"device"`` raises
    ``ValueError`` for a ``.gz`` file that is not BGZF; a plain file is read plainly in every mode."""
    if inflate not in INFLATE_MODES:
        raise ValueError("inflate must be one of %s, not %r" % (", ".join(repr(m) for m in INFLATE_MODES), inflate))
    if inflate == "host" or not str(path).endswith(".gz"):
        return False
    if is_bgzf(path):
        return True
    if inflate == "device":
        raise ValueError("%s: not a BGZF file (inflate=\"device\" takes bgzip's format only; inflate=\"host\" reads any "
                         "gzip file)" % path)
    return False


def need_chunks(inflate: str, chunked: bool, what: str) -> None:
    """``inflate`` other than "host" belongs to the streamed routes: the whole-file routes read ``text()``."""
    if inflate not in INFLATE_MODES:
        raise ValueError("inflate must be one of %s, not %r" % (", ".join(repr(m) for m in INFLATE_MODES), inflate))
    if inflate != "host" and not chunked:
        raise ValueError("inflate=%r applies to files that are streamed: set %s" % (inflate, what))


def open_source(path: str, inflate: str, host_open):
    """The byte source of ``path`` for a streamed route: a ``BgzfSource`` when ``inflate`` sends the file's compressed
    bytes to the device (``use_device_inflate``), else what ``host_open()`` gives — the route's source of today."""
    return BgzfSource(path) if use_device_inflate(path, inflate) else host_open()


class Chunk(NamedTuple):
    """One staged chunk of a ``BgzfSource``.  ``comp_len`` compressed bytes are staged, the whole members of ``table``
    (text offsets from 0, ``text_new`` bytes of text in all).  The chunk's text, ``text_len`` bytes, is the first
    ``take`` bytes of the remainder — what the previous chunks' last member left over — and then the members' text as
    far as the chunk goes; the new remainder, ``keep`` bytes, is what the old one has beyond ``take`` (``rest``
    bytes) or what the members' text has beyond the chunk, never both."""
    comp_len: int
    table: np.ndarray
    take: int
    rest: int
    text_new: int
    text_len: int
    keep: int
    final: bool


def assemble(chunk: Chunk, remainder: bytes, new_text: bytes) -> Tuple[bytes, bytes]:
    """What the device does with a chunk, on bytes: (the chunk's text, the new remainder) from the old remainder and
    the inflated text of the chunk's members."""
    assert len(remainder) == chunk.take + chunk.rest and len(new_text) == chunk.text_new
    got = chunk.text_len - chunk.take
    text = remainder[:chunk.take] + new_text[:got]
    keep = remainder[chunk.take:] + new_text[got:]
    assert len(text) == chunk.text_len and len(keep) == chunk.keep and (chunk.rest == 0 or chunk.text_new == got)
    return text, keep


class BgzfSource:
    """A BGZF file as a source whose staged bytes are inflated on the device: ``stage_compressed(view, nbytes)`` puts
    the whole members that hold the next ``nbytes`` of text, less what the remainder holds, into ``view`` and says how
    the chunk's text is put together (``Chunk``).  The empty members behind a chunk's last member — the end-of-file
    marker — go with it.  End of file is known from the walk, where no member with ISIZE > 0 is left, not from a byte
    read ahead; like ``gzip.open`` it raises ``EOFError`` for a file that ends inside a member, and ``ValueError`` for
    a member that is not BGZF, when the chunk cannot be had, or ends, in front of it."""
    READ = 1 << 20

    def __init__(self, path: str):
        self.name = str(path)
        self._f = open(self.name, "rb", buffering=0)
        self._buf = bytearray()      # compressed bytes read and not yet staged
        self._file_pos = 0           # file offset of _buf[0]
        self._at_file_end = False
        self.left = 0                # bytes of the remainder
        self.final = False

    @staticmethod
    def staging_bytes(chunk_bytes: int) -> int:
        """Bytes of a staging block, and of a slot's compressed buffer, for chunks of ``chunk_bytes`` of text: DEFLATE
        grows text by five bytes in 64 KiB at the most and BGZF by 26 a member; the member a chunk ends in comes whole.
        (A file of members of a few bytes each needs more: ``stage_compressed`` says so.)"""
        return chunk_bytes + chunk_bytes // 8 + 4 * MAX_TEXT

    def close(self) -> None:
        self._f.close()

    def __enter__(self) -> "BgzfSource":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def _walk(self, budget: int) -> Walk:
        """The members at the front of the file's unstaged bytes, up to ``budget`` bytes of text, reading on until the
        walk stops for the budget, for a member that is not BGZF, or at the end of the file."""
        while True:
            a = np.frombuffer(self._buf, dtype=np.uint8)
            w = walk_blocks(a, self._file_pos, budget)
            del a     # (the bytearray grows below)
            if w.why not in (WALK_END, WALK_INSIDE) or self._at_file_end:
                return w
            got = self._f.read(self.READ)
            if got:
                self._buf += got
            else:
                self._at_file_end = True

    def stage_compressed(self, view, nbytes: int) -> Chunk:
        none = np.empty((0, ROW), dtype=np.int64)
        if self.final:
            return Chunk(0, none, 0, 0, 0, 0, 0, True)
        left = self.left
        take = min(left, nbytes)
        need = nbytes - take                     # bytes of text the members have to bring
        w = self._walk(need + MAX_TEXT)          # (the member in which `need` is reached starts before it)
        ends = w.table[:, 2] + w.table[:, 3]
        reached = w.text_bytes >= need
        k = (int(np.searchsorted(ends, need, "left")) + 1 if need > 0 else 0) if reached else w.members
        while k < w.members and w.table[k, 3] == 0:
            k += 1
        text_new = int(ends[k - 1]) if k else 0
        got = min(need, text_new)
        keep = (left - take) + (text_new - got)
        blocked = k == w.members                 # nothing is known of what follows the chunk's members
        if blocked and (keep == 0 or not reached):
            if w.why == WALK_NOT_BGZF:
                raise ValueError("%s: no BGZF member at offset %d (inflate=\"host\" reads any gzip file)"
                                 % (self.name, self._file_pos + w.stop))
            if w.why == WALK_INSIDE:
                raise EOFError("Compressed file ended before the end-of-stream marker was reached: %s" % self.name)
        comp_len = int(w.table[k, 5]) - self._file_pos if k < w.members else w.comp_bytes
        if comp_len > len(view):
            raise _lib.GfError(_lib.GF_ERR_CAPACITY, "%s: the members of a chunk take %d bytes, the staging block has %d "
                               "(members of very little text each); inflate=\"host\" reads it" % (self.name, comp_len, len(view)))
        view[:comp_len] = self._buf[:comp_len]
        del self._buf[:comp_len]
        self._file_pos += comp_len
        self.left = keep
        self.final = blocked and keep == 0 and w.why == WALK_END
        return Chunk(comp_len, w.table[:k].copy(), take, left - take, text_new, take + got, keep, self.final)


class DeviceInflate:
    """The device half of one inflating side of a ``ChunkStream``: a compressed buffer per slot and the remainder."""

    def __init__(self, source: BgzfSource, chunk_bytes: int, dev):
        import torch
        self.source = source
        self.comp = [torch.empty(source.staging_bytes(chunk_bytes), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.remainder = torch.empty(MAX_TEXT, dtype=torch.uint8, device=dev)

    def upload(self, slot: int, chunk: Chunk, host_ptr: int, text, copy_stream) -> None:
        """The chunk's text into ``text`` — the slot's text buffer behind its room for the carry, with MAX_TEXT of room
        behind a chunk — on ``copy_stream``, from an upload thread: the staged bytes cross the link, the remainder
        comes first, the members are inflated behind it and what they have beyond the chunk becomes the remainder.
        Ends with the stream's synchronise and the totals' read-back; raises ``gzip.BadGzipFile`` for a member that
        fails."""
        import torch
        n, take, rest = chunk.table.shape[0], chunk.take, chunk.rest
        totals = None
        with torch.cuda.stream(copy_stream):
            comp = self.comp[slot][:chunk.comp_len]
            if chunk.comp_len:
                check(lib().gf_if_copy_from_host_device(host_ptr, comp.data_ptr(), chunk.comp_len, copy_stream.cuda_stream))
            if take:
                text[:take].copy_(self.remainder[:take])
            if rest:
                self.remainder[:rest].copy_(self.remainder[take:take + rest].clone())
            if n:
                out = text[take:take + chunk.text_new]
                _, totals = inflate_device(comp, torch.from_numpy(chunk.table).to(text.device), out)
                got = chunk.text_len - take
                if chunk.text_new > got:
                    self.remainder[:chunk.text_new - got].copy_(out[got:])
            copy_stream.synchronize()
            if totals is not None:
                _, first, status, _ = (int(x) for x in totals.cpu())
                if first >= 0:
                    raise gzip.BadGzipFile("%s: BGZF member at offset %d: %s" % (
                        self.source.name, int(chunk.table[first, 5]), STATUS_TEXT.get(status, "status %d" % status)))
