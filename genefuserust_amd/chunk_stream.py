"""A file through the device in chunks: the double-buffered loop of the streamed FASTQ scans (scan_stream.py) and of
the reference cut (ref_cut.py).

    byte sources (files, gunzipped as they are read; texts in memory)  --readinto, upload threads-->  pinned staging
    blocks  --H2D, copy stream-->  device text buffers (behind the carried-over tail of the previous chunk)  -->
    (or: BGZF files, compressed as they are  -->  staging blocks  --H2D-->  inflated into the text buffers: bgzf.py)
    the consumer's ``process(texts, final)`` on the processing stream  -->  how many bytes of each text are done with.

``ChunkStream`` owns the streams, the slots, the threads and the carries; what a chunk means, and when to stop before the
sources end, is the consumer's.  ``read_chunk``, ``Side.stage`` and the read-size rules need no GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading
import time
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .bgzf import DeviceInflate

CARRY_MAX = 1 << 20  # bytes kept in front of a chunk for the previous chunk's tail


class ArraySource:
    """A byte source over a text held as a uint8 array.  ``readinto`` is what every source has; an array also lends its
    bytes where they are (``take``), so that a pinned text crosses the link without a copy on the host."""
    name = "<memory>"

    def __init__(self, text: np.ndarray):
        assert text.dtype == np.uint8 and text.ndim == 1
        self.text = text
        self.pos = 0

    def take(self, nbytes: int) -> np.ndarray:
        """The next (at most) ``nbytes`` bytes as a view of the array."""
        n = int(max(0, min(nbytes, self.text.size - self.pos)))
        out = self.text[self.pos:self.pos + n]
        self.pos += n
        return out

    def at_end(self) -> bool:
        return self.pos >= self.text.size

    def readinto(self, mv) -> int:
        src = self.take(len(mv))
        np.frombuffer(mv, dtype=np.uint8)[:src.size] = src
        return int(src.size)


def read_chunk(source, view, nbytes: int, ahead: bytes) -> Tuple[int, bytes, bool]:
    """Fill ``view`` with ``ahead`` (what the previous call read past its chunk) and the next bytes of ``source`` up to
    ``nbytes`` in all (fewer at the source's end), then read one byte ahead to see whether the source has ended.
    Returns (bytes in the view, the byte read ahead or b"", whether the source's last byte is in this chunk)."""
    n = len(ahead)
    view[:n] = ahead
    while n < nbytes:
        got = source.readinto(view[n:nbytes])
        if not got:
            return n, b"", True
        n += got
    one = bytearray(1)
    if source.readinto(memoryview(one)):
        return n, bytes(one), False
    return n, b"", True


def fill_read_sizes(chunk_bytes: int, sides: Sequence[Tuple[int, bool]]) -> List[int]:
    """The FASTQ rule, per side (carry_len, starved): what fills the chunk behind the carry, so that the file that is
    ahead (longer carry) gets fewer new bytes."""
    # (a side whose carry alone fills a chunk is either ahead of the other file — it waits, a byte at a time — or
    #  in the middle of a record longer than a chunk, which needs the next chunk whole)
    return [chunk_bytes - carry if carry < chunk_bytes else (chunk_bytes if starved else 1) for carry, starved in sides]


def whole_read_sizes(chunk_bytes: int, sides: Sequence[Tuple[int, bool]]) -> List[int]:
    """The reference cut's rule: ``chunk_bytes`` whatever was carried."""
    return [chunk_bytes for _ in sides]


def checked_chunk_bytes(chunk_bytes) -> int:
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be positive, not %r" % (chunk_bytes,))
    return chunk_bytes


class Side:
    """The host half of one text: a byte source — anything with ``readinto(memoryview) -> int``, 0 at the end — and the
    two staging blocks its chunks are read into: pinned ones of ``gf_host_alloc``, or the writable ``views`` given (a
    test's bytearrays).  A source that lends its bytes (``take``) needs none.  A source whose staged bytes are inflated
    on the device (``stage_compressed``, bgzf.BgzfSource) stages compressed bytes, whole members, in blocks of the size
    it asks for, and says how the chunk's text is put together (``chunks[slot]``)."""

    def __init__(self, source, chunk_bytes: int, views=None):
        self.source = source
        self.name = getattr(source, "name", "<stream>")
        self.lends = hasattr(source, "take")
        self.inflates = hasattr(source, "stage_compressed")
        self.chunk_len = [0, 0]
        self.chunks: list = [None, None]   # (an inflating source's bgzf.Chunk per slot)
        self.eof = False      # the source's last byte is in a chunk staged so far
        self.ahead = b""      # the byte read past a full chunk to see whether the source has ended
        self.staging: List[int] = []
        self.views: list = [] if views is None else list(views)
        if views is None and not self.lends:
            L = _lib.lib()
            block = source.staging_bytes(chunk_bytes) if self.inflates else chunk_bytes
            for _ in range(2):
                p = L.gf_host_alloc(block)
                if not p:
                    self.close()
                    raise _lib.GfError(_lib.GF_ERR_HIP, "gf_host_alloc(%d) failed" % block)
                self.staging.append(p)
                self.views.append(memoryview((C.c_uint8 * block).from_address(p)).cast("B"))

    def close(self) -> None:
        self.views = []
        for p in self.staging:
            _lib.lib().gf_host_free(p)
        self.staging = []

    def stage(self, slot: int, nbytes: int) -> Tuple[Optional[int], int]:
        """The next ``nbytes`` of the source (fewer at its end, none after it) where a copy to the device can take them:
        (address — None for views that were given —, length); sets ``chunk_len[slot]`` and ``eof``.  Runs on an upload
        thread: reading (and gunzipping) blocks that thread only."""
        ptr, n = None, 0
        if self.eof:
            self.chunks[slot] = None
        elif self.lends:
            src = self.source.take(nbytes)
            ptr, n = src.ctypes.data, int(src.size)
            self.eof = self.source.at_end()
        elif self.inflates:     # (ptr, n: the compressed bytes staged; chunk_len is the text's)
            c = self.chunks[slot] = self.source.stage_compressed(self.views[slot], nbytes)
            self.chunk_len[slot], self.eof = c.text_len, c.final
            return (self.staging[slot] if self.staging else None), c.comp_len
        else:
            n, self.ahead, self.eof = read_chunk(self.source, self.views[slot], nbytes, self.ahead)
            ptr = self.staging[slot] if self.staging else None
        self.chunk_len[slot] = n
        return ptr, n


class ChunkStream:
    """``sources`` streamed through ``dev`` in chunks of ``chunk_bytes``: chunk k + 1 is read and crosses the link while
    chunk k is processed.  ``copy(host address, device address, nbytes, stream handle)`` queues one H2D copy — through a
    library's own hipMemcpyAsync: torch only treats memory of its own pinned allocator as pinned, and copies from
    anything else (gf_host_alloc memory included) synchronously.  ``read_sizes(chunk_bytes, [(carry_len, starved), ..])``
    says how many bytes each side reads next.  The host holds two staging blocks per side, the device two text buffers
    of ``CARRY_MAX + chunk_bytes`` per side."""

    def __init__(self, sources, chunk_bytes: int, dev, copy: Callable, read_sizes: Callable):
        import torch
        chunk_bytes = checked_chunk_bytes(chunk_bytes)
        self.chunk_bytes, self.dev, self.copy, self.read_sizes = chunk_bytes, dev, copy, read_sizes
        self.copy_stream = torch.cuda.Stream(dev)
        # The chunks are processed on a stream of their own, not on the legacy null stream: the null stream and
        # the other streams wait for each other, and an upload in flight then stalls every kernel of the chunk
        # being processed (measured: 9.4 ms of upload + 7 ms of processing per 2 x 256 MB, one after the other).
        self.proc = torch.cuda.Stream(dev)
        self.free = [None, None]      # per slot: event after which the slot's buffers may be overwritten
        self.threads: list = [None, None]
        self.errors: List[BaseException] = []   # of the upload threads, handed to the consumer by _wait_upload
        self.sides: List[Side] = []
        self.bufs: list = []          # per side, per slot
        self.carry_len: List[int] = []
        self.starved: List[bool] = []
        self.inflate: list = []       # per side: its bgzf.DeviceInflate, or None
        try:
            for src in sources:
                inflates = hasattr(src, "stage_compressed")
                # (an inflated chunk's last member is written whole: up to 64 KiB of room behind the chunk)
                room = (1 << 16) if inflates else 0
                self.bufs.append([torch.empty(CARRY_MAX + chunk_bytes + 64 + room, dtype=torch.uint8, device=dev)
                                  for _ in range(2)])
                self.sides.append(Side(src, chunk_bytes))
                self.inflate.append(DeviceInflate(src, chunk_bytes, dev) if inflates else None)
                self.carry_len.append(0)
                self.starved.append(True)
        except BaseException:
            self.close()
            raise

    def close(self) -> None:
        import torch
        for th in self.threads:
            if th is not None:
                th.join()
        torch.cuda.synchronize(self.dev)   # (no copy in flight out of the staging blocks)
        for s in self.sides:
            s.close()

    def _start_upload(self, slot: int) -> None:
        """The slot's next chunk, on host threads of their own, one per side: reading the source (gunzip included) and
        the calls that queue the copy block those threads, not the one that launches the kernels of the chunk being
        processed — and R1 and R2 are read at the same time."""
        import torch
        # (the carry lengths read here are those of the chunk processed LAST, not of the one in flight: the balancing
        #  of the two files lags one chunk behind — harmless, a slot always has room for chunk_bytes behind CARRY_MAX)
        nbytes = self.read_sizes(self.chunk_bytes, list(zip(self.carry_len, self.starved)))
        wait_for = self.free[slot]

        def guarded(fn, *args):
            try:
                torch.cuda.set_device(self.dev)
                fn(*args)
            except BaseException as e:   # (handed to the consumer by _wait_upload)
                self.errors.append(e)

        def one(k: int):
            ptr, n = self.sides[k].stage(slot, nbytes[k])
            if self.sides[k].chunks[slot] is not None:
                self.inflate[k].upload(slot, self.sides[k].chunks[slot], ptr, self.bufs[k][slot][CARRY_MAX:],
                                       self.copy_stream)
            elif n:
                self.copy(ptr, self.bufs[k][slot].data_ptr() + CARRY_MAX, n, self.copy_stream.cuda_stream)

        def run():
            if wait_for is not None:
                wait_for.synchronize()
            others = [threading.Thread(target=guarded, args=(one, k)) for k in range(1, len(self.sides))]
            for th in others:
                th.start()
            guarded(one, 0)
            for th in others:
                th.join()
            self.copy_stream.synchronize()
        self.threads[slot] = threading.Thread(target=guarded, args=(run,))
        self.threads[slot].start()

    def _wait_upload(self, slot: int) -> None:
        self.threads[slot].join()
        if self.errors:
            raise self.errors[0]

    def run(self, process: Callable):
        """The chunk loop, a generator.  Per chunk, on the processing stream and with the carries already in front:
        ``process(texts, final) -> (used, starved, result)`` — ``texts`` the sides' device texts, ``final[k]`` whether
        side k's last byte is in this (or an earlier) chunk; ``used[k]`` how many bytes of text k are done with (the
        rest, at most ``CARRY_MAX``, is carried to the front of the next chunk), ``starved[k]`` for ``read_sizes`` —
        and yields ``result``.  Ends after the chunk in which every side is final, or when the consumer closes it;
        either way it joins the threads, synchronises the device and frees the staging blocks."""
        import torch
        try:
            carries = [torch.empty(0, dtype=torch.uint8, device=self.dev) for _ in self.sides]
            slot = 0
            self._start_upload(0)
            while True:
                t_a = time.perf_counter()
                self._wait_upload(slot)                  # this chunk's text is on the device
                t_b = time.perf_counter()
                final = [s.eof for s in self.sides]
                if not all(final):
                    self._start_upload(slot ^ 1)         # the next chunk is read and crosses the link meanwhile
                with torch.cuda.stream(self.proc):
                    texts = []
                    for bufs, s, c in zip(self.bufs, self.sides, carries):
                        n0, buf = c.numel(), bufs[slot]
                        if n0:
                            buf[CARRY_MAX - n0:CARRY_MAX].copy_(c)
                        texts.append(buf[CARRY_MAX - n0:CARRY_MAX + s.chunk_len[slot]])
                    used, self.starved, result = process(texts, final)
                    carries = [t[u:].clone() for t, u in zip(texts, used)]
                    self.carry_len = [int(c.numel()) for c in carries]
                    self.free[slot] = torch.cuda.Event()
                    self.free[slot].record(self.proc)
                if os.environ.get("GF_STREAM_DEBUG") == "1":
                    print("chunk: waited %.2f ms for its upload, processed in %.2f ms"
                          % (1e3 * (t_b - t_a), 1e3 * (time.perf_counter() - t_b)), file=sys.stderr, flush=True)
                yield result
                if all(final):
                    break
                slot ^= 1
        finally:
            self.close()
