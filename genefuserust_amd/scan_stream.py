"""The scans as a stream of FASTQ text: ``PairEndScanner::scan`` / ``SingleEndScanner::scan`` read their files in
packs while the consumers map them (src/core/pescanner.rs:255-395, sescanner.rs:62-181); here the host hands over raw
text chunks — any byte boundaries, it does not parse — and everything from the records to the hit
list happens on the device, chunk k+1 being read and crossing the link while chunk k is processed:

    byte source (a file, gunzipped as it is read; a text in memory)  --readinto, upload threads-->  pinned staging
    block  --H2D, copy stream-->  device text buffer (behind the carried-over tail of the previous chunk)  -->
    gf_fastq_index_device / gf_fastq_gather_device  -->  gf_scan_pairs_device (merge, map, reverse-complement
    retries, ordered compaction) or gf_se_scan_device  -->  gf_hn_names_device (the names of the hit records)  -->
    gf_pair_hit records + their reads + their names, back to the host; gf_pair_hits_finish there.

A chunk ends anywhere; the bytes after its last complete record (of the record count both files
share) are carried to the front of the next chunk on the device.  A few tiny read-backs per chunk
(the line counts, the carry positions) are the only synchronisation before the results.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading
import time
from typing import Iterator, List, Optional, Tuple

import numpy as np

from . import _lib
from .fusion_mapper import FusionMapper, ReadMatch
from .indexer import Indexer
from .read_pair import finish_pair_hits, scan_pairs_device, scan_with_room

CARRY_MAX = 1 << 20  # bytes kept in front of a chunk for the previous chunk's tail


class ArraySource:
    """A byte source over a FASTQ text held as a uint8 array.  ``readinto`` is what every source has; an array also
    lends its bytes where they are (``take``), so that a pinned text crosses the link without a copy on the host."""
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


class _Side:
    """One FASTQ text: a byte source — anything with ``readinto(memoryview) -> int``, 0 at the end — two pinned staging
    blocks its chunks are read into, and two device buffers the chunks alternate between."""

    def __init__(self, source, chunk_bytes: int, dev, handle):
        import torch
        self.h = handle
        self.source = source
        self.name = getattr(source, "name", "<stream>")
        self.bufs = [torch.empty(CARRY_MAX + chunk_bytes + 64, dtype=torch.uint8, device=dev) for _ in range(2)]
        self.carry_len = 0
        self.starved = True
        self.chunk_len = [0, 0]
        self.eof = False
        self.ahead = b""      # the byte read past a full chunk to see whether the source has ended
        self.staging: List[int] = []
        self.views: list = []
        if not hasattr(source, "take"):
            L = _lib.lib()
            for _ in range(2):
                p = L.gf_host_alloc(chunk_bytes)
                if not p:
                    self.close()
                    raise _lib.GfError(_lib.GF_ERR_HIP, "gf_host_alloc(%d) failed" % chunk_bytes)
                self.staging.append(p)
                self.views.append(memoryview((C.c_uint8 * chunk_bytes).from_address(p)).cast("B"))

    def close(self) -> None:
        self.views = []
        for p in self.staging:
            _lib.lib().gf_host_free(p)
        self.staging = []

    def done(self) -> bool:
        return self.eof

    def _read(self, slot: int, nbytes: int) -> int:
        """Fill the slot's staging block with the next ``nbytes`` of the source (fewer at its end); sets ``eof``."""
        mv = self.views[slot]
        n = len(self.ahead)
        mv[:n] = self.ahead
        self.ahead = b""
        while n < nbytes:
            got = self.source.readinto(mv[n:nbytes])
            if not got:
                self.eof = True
                return n
            n += got
        one = bytearray(1)
        if self.source.readinto(memoryview(one)):
            self.ahead = bytes(one)
        else:
            self.eof = True
        return n

    def upload(self, slot: int, nbytes: int, stream) -> None:
        """Read the next ``nbytes`` of the source and queue their H2D copy into buffer ``slot`` (after the carry
        area).  Runs on an upload thread: reading (and gunzipping) blocks that thread only."""
        if self.eof:
            self.chunk_len[slot] = 0
            return
        if self.staging:
            n = self._read(slot, nbytes)
            ptr = self.staging[slot]
        else:
            src = self.source.take(nbytes)
            n, ptr = int(src.size), src.ctypes.data
            self.eof = self.source.at_end()
        self.chunk_len[slot] = n
        if n:
            self._copy(ptr, self.bufs[slot].data_ptr() + CARRY_MAX, n, stream.cuda_stream)

    def _copy(self, ptr: int, dst: int, n: int, stream: int) -> None:
        # through the library's own hipMemcpyAsync: torch only treats memory of its own pinned allocator as
        # pinned, and copies from anything else (gf_host_alloc memory included) synchronously
        _lib.check(_lib.lib().gf_copy_from_host_device(self.h, ptr, dst, n, stream))


def _scan_source_stream(indexer: Indexer, sources, chunk_bytes: int, max_read_len: Optional[int], names: bool):
    """The chunk loop of both layouts: ``sources`` is (R1, R2) or (reads,).  Yields per chunk (records, hit bases, hit
    qualities, names or None, totals)."""
    import torch
    from .fastq import fastq_cut_device
    from .hit_names import hit_names_device
    from .single_end import scan_single_device
    single = len(sources) == 1
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError("chunk_bytes must be positive, not %r" % (chunk_bytes,))
    dev = torch.device("cuda", indexer.info()["device"])
    copy_stream = torch.cuda.Stream(dev)
    sides: List[_Side] = []
    free = [None, None]    # per slot: event after which the slot's buffers may be overwritten

    upload_threads = [None, None]
    upload_errors: List[BaseException] = []

    def start_upload(slot: int):
        """The slot's next chunk, on host threads of their own, one per side: reading the source (gunzip included) and
        the calls that queue the copy block those threads, not the one that launches the kernels of the chunk being
        processed — and R1 and R2 are read at the same time."""
        # (the carry lengths read here are those of the chunk processed LAST, not of the one in flight: the balancing
        #  of the two files lags one chunk behind — harmless, a slot always has room for chunk_bytes behind CARRY_MAX)
        # (a side whose carry alone fills a chunk is either ahead of the other file — it waits, a byte at a time — or
        #  in the middle of a record longer than a chunk, which needs the next chunk whole)
        nbytes = [chunk_bytes - s.carry_len if s.carry_len < chunk_bytes else (chunk_bytes if s.starved else 1)
                  for s in sides]
        wait_for = free[slot]

        def one(s: _Side, nb: int):
            try:
                torch.cuda.set_device(dev)
                s.upload(slot, nb, copy_stream)   # the file that is ahead (longer carry) gets fewer new bytes
            except BaseException as e:   # (handed to the consumer by wait_upload)
                upload_errors.append(e)

        def run():
            torch.cuda.set_device(dev)
            if wait_for is not None:
                wait_for.synchronize()
            others = [threading.Thread(target=one, args=(s, nb)) for s, nb in zip(sides[1:], nbytes[1:])]
            for th in others:
                th.start()
            one(sides[0], nbytes[0])
            for th in others:
                th.join()
            copy_stream.synchronize()
        th = threading.Thread(target=run)
        th.start()
        upload_threads[slot] = th

    def wait_upload(slot: int):
        upload_threads[slot].join()
        if upload_errors:
            raise upload_errors[0]

    done = 0
    slot = 0
    # The chunks are processed on a stream of their own, not on the legacy null stream: the null stream and
    # the other streams wait for each other, and an upload in flight then stalls every kernel of the chunk
    # being processed (measured: 9.4 ms of upload + 7 ms of processing per 2 x 256 MB, one after the other).
    proc = torch.cuda.Stream(dev)

    def process(slot: int, final, carries, done: int):
        """One chunk on the stream `proc`: (result or None, new carries, counts, m)."""
        texts = []
        for s, c in zip(sides, carries):
            n0 = c.numel()
            buf = s.bufs[slot]
            if n0:
                buf[CARRY_MAX - n0:CARRY_MAX].copy_(c)
            texts.append(buf[CARRY_MAX - n0:CARRY_MAX + s.chunk_len[slot]])
        # records of the texts (device).  A side whose last byte has arrived counts its unterminated last
        # line (fastq_reader.rs:75-147); the others only the lines that end inside the chunk.
        # (pairs, lean: the qualities stay in the chunk's text, which lives in the slot's buffer until the scan below is
        #  done; single-end: gf_se_scan_device takes the qualities at the bases' offsets, so the full cut)
        batches = [fastq_cut_device(indexer, t, lean=not single) for t in texts]
        counts = [b.n_records if f else b.n_newlines // 4 for b, f in zip(batches, final)]
        m = min(counts)
        new_carries = []
        for s, b, t in zip(sides, batches, texts):
            if m == 0:
                cut = 0
            elif 4 * m - 1 < b.n_newlines:
                cut = int(b.nl_pos[4 * m - 1].item()) + 1
            else:   # record m-1 ends with the text (no final newline)
                cut = t.numel()
            tail = t[cut:]
            if tail.numel() > CARRY_MAX:
                raise _lib.GfError(_lib.GF_ERR_CAPACITY, "%s: a FASTQ chunk left more than %d bytes for the next one: a "
                                   "record does not fit, or the two files' records drift apart faster than the chunks "
                                   "can absorb" % (s.name, CARRY_MAX))
            new_carries.append(tail.clone())
            s.carry_len = int(tail.numel())
        for s, c in zip(sides, counts):
            s.starved = c == m   # every complete record of this side was used: the other side is not behind it
        out = None
        if m > 0:
            offs = [b.offsets[:m + 1] for b in batches]
            nb = [int(o[-1].item()) for o in offs]
            mrl = max_read_len
            if mrl is None:   # the longest read of the chunk, as the whole-file scans take the longest of the file
                mrl = max([int((o[1:] - o[:-1]).max().item()) for o in offs] + [1])
            if single:
                b = batches[0]

                def scan(**caps):
                    return scan_single_device(indexer, b.bases[:nb[0]], b.quals[:nb[0]], offs[0], mrl,
                                              read_id_base=done, **caps)
                room = dict(hits_cap=m, bytes_cap=nb[0] + 64, retry_cap=m)
            else:
                l, r = batches
                lean = l.qual_off is not None and r.qual_off is not None
                if not lean:   # one side has a quality line of another length than its sequence: both the full way
                    l = l if l.qual_off is None else fastq_cut_device(indexer, texts[0])
                    r = r if r.qual_off is None else fastq_cut_device(indexer, texts[1])
                lq, rq = (l.quals, r.quals) if lean else (l.quals[:nb[0]], r.quals[:nb[1]])
                qo = dict(l_qual_off=l.qual_off[:m], r_qual_off=r.qual_off[:m]) if lean else {}

                def scan(**caps):
                    return scan_pairs_device(indexer, l.bases[:nb[0]], lq, offs[0], r.bases[:nb[1]], rq, offs[1], mrl,
                                             pair_id_base=done, **caps, **qo)
                room = dict(hits_cap=3 * m, bytes_cap=2 * sum(nb) + 64, retry_cap=3 * m)

            def gather(res, **cap):
                return hit_names_device(indexer, res, texts[0], batches[0], *(() if single else (texts[1], batches[1])),
                                        pair_id_base=done, **cap) if names else None
            # (first with the library's default capacities; the names are queued behind the scan: the record count
            #  stays on the device)
            res, nm, out = scan_with_room(scan, {}, room, gather)
            name_list = None
            if names:
                _, need, over, _ = (int(x) for x in nm.totals.cpu())
                if over:   # names longer than 64 bytes on average: once more with the room the first call asked for
                    nm = gather(res, names_cap=need)
                name_list = nm.download()
            out[3]["reads" if single else "pairs"] = m
            out = (out[0], out[1], out[2], name_list, out[3])
        ev = torch.cuda.Event()
        ev.record(proc)
        free[slot] = ev
        return out, new_carries, counts, m

    try:
        for src in sources:
            sides.append(_Side(src, chunk_bytes, dev, indexer._handle()))
        carries = [torch.empty(0, dtype=torch.uint8, device=dev) for _ in sides]
        start_upload(0)
        while True:
            t_a = time.perf_counter()
            wait_upload(slot)                   # this chunk's text is on the device
            t_b = time.perf_counter()
            final = [s.done() for s in sides]   # the side's last byte is in this (or an earlier) chunk
            if not all(final):
                start_upload(slot ^ 1)          # the next chunk is read and crosses the link while this one is processed
            with torch.cuda.stream(proc):
                out, carries, counts, m = process(slot, final, carries, done)
            if os.environ.get("GF_STREAM_DEBUG") == "1":
                print("chunk: waited %.2f ms for its upload, processed in %.2f ms" % (1e3 * (t_b - t_a), 1e3 * (time.perf_counter() - t_b)),
                      file=sys.stderr, flush=True)
            if out is not None:
                yield out
            done += m
            # records pair up by position and the shorter file ends both (fastq_reader.rs:209-218): stop when a
            # side that has all its bytes has no record left
            if all(final) or any(f and c == m for f, c in zip(final, counts)):
                break
            slot ^= 1
    finally:
        for th in upload_threads:
            if th is not None:
                th.join()
        torch.cuda.synchronize(dev)   # (no copy in flight out of the staging blocks)
        for s in sides:
            s.close()


def scan_pair_source_stream(indexer: Indexer, r1_source, r2_source, chunk_bytes: int = 128 << 20,
                            max_read_len: Optional[int] = 320,
                            names: bool = True) -> Iterator[Tuple[np.ndarray, bytes, bytes, Optional[List[bytes]], dict]]:
    """The paired-end scan of two byte sources of FASTQ text — anything with ``readinto(memoryview) -> int`` (0 at
    the end): ``ArraySource``, ``fastq.FastqReader.open_stream()`` — chunk by chunk.  Yields, per chunk, (gf_pair_hit
    records with pair ids counted from the start of the files, the matched reads' bases, their qualities, the names of
    the records' reads (``hit_names_device``; None with ``names=False``), totals); ``totals["pairs"]`` is the chunk's
    pair count.  Records pair up by position; the shorter file ends both (fastq_reader.rs:209-218).  The next chunk of
    each source is read (gunzipped) and uploaded on host threads while the device works on the current one; the host
    holds two staging blocks of ``chunk_bytes`` per side.  ``max_read_len=None``: the longest read of each chunk."""
    return _scan_source_stream(indexer, (r1_source, r2_source), chunk_bytes, max_read_len, names)


def scan_pair_text_stream(indexer: Indexer, r1_text: np.ndarray, r2_text: np.ndarray, chunk_bytes: int = 128 << 20,
                          max_read_len: int = 320) -> Iterator[Tuple[np.ndarray, bytes, bytes, dict]]:
    """Yields, per chunk, what ``PairScan.download`` returns — (gf_pair_hit records with pair ids counted
    from the start of the files, the matched reads' bases, their qualities, totals) — for the FASTQ
    texts ``r1_text`` / ``r2_text`` (uint8 arrays; pinned memory makes the copies asynchronous).
    Records pair up by position; the shorter file ends both (fastq_reader.rs:209-218)."""
    for rec, hb, hq, _, tot in scan_pair_source_stream(indexer, ArraySource(r1_text), ArraySource(r2_text), chunk_bytes,
                                                       max_read_len, names=False):
        yield rec, hb, hq, tot


def scan_single_text_stream(indexer: Indexer, source, chunk_bytes: int = 128 << 20, max_read_len: Optional[int] = 320,
                            names: bool = True) -> Iterator[Tuple[np.ndarray, bytes, bytes, Optional[List[bytes]], dict]]:
    """The single-end counterpart: one byte source (a uint8 array is wrapped into an ``ArraySource``), scanned chunk by
    chunk with ``single_end.scan_single_device`` (``read_id_base`` = reads done so far).  Yields per chunk (records, hit
    bases, hit qualities, names, totals); ``totals["reads"]`` is the chunk's record count.  A final record without a
    trailing newline counts (fastq_reader.rs:75-147)."""
    if isinstance(source, np.ndarray):
        source = ArraySource(source)
    return _scan_source_stream(indexer, (source,), chunk_bytes, max_read_len, names)


def scan_pair_end_text(indexer: Indexer, r1_text: np.ndarray, r2_text: np.ndarray, chunk_bytes: int = 128 << 20,
                       threads: int = 8) -> Tuple[List[Tuple[int, ReadMatch]], dict]:
    """The whole paired-end scan of two FASTQ texts up to the ReadMatch list (before the filters):
    ([(pair index, ReadMatch)] in push order, counters)."""
    mapper = FusionMapper(indexer)
    found: List[Tuple[int, ReadMatch]] = []
    counters = {"pairs": 0, "merged_pairs": 0, "retried_reads": 0, "hits": 0, "chunks": 0}
    for rec, hb, hq, tot in scan_pair_text_stream(indexer, r1_text, r2_text, chunk_bytes):
        found += finish_pair_hits(mapper, rec, hb, hq, threads)
        for k in ("pairs", "merged_pairs", "retried_reads", "hits"):
            counters[k] += tot[k]
        counters["chunks"] += 1
    return found, counters
