"""The cleaned reads written out as FASTQ files, formatted on the device, opt-in: the ``gf_rw_*`` calls of
libgfwrite.so (include/gf_read_write.h, which states the predicate).

The UMI cut, the adapter trimming, the read filter and the duplicate removal leave the records they pass in HBM for
the length of one chunk, and only the scan sees them.  A pipeline's other tools — an aligner, a variant caller — want
the same records as files, and an inline UMI that was cut off is gone unless it is written into the name of the record
that leaves.  ``ReadWriter`` writes them: per chunk one call formats the records that are left with bases (for pairs:
both mates) as FASTQ text where they are, one device-to-host copy per side brings the text into a pinned staging block,
and a thread per file writes it, compressed by the host's zlib for a name that ends in ``.gz``.  A feature outside the
reference, off unless a ``ReadWriter`` is handed to a streamed route.  libgfwrite.so is a library of its own on top of
libgfmatch.so's public C ABI (genefuserust_amd/scan_csrc/).  No CPU fallback: without the libraries and a GPU every
device call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import threading
import zlib
from typing import NamedTuple, Optional, Sequence

from . import _lib

RW_LIB_PATH = os.path.join(_lib._HERE, "libgfwrite.so")

TAG_MAX, TOTALS = 1 + 32 + 1 + 32, 5
WIDE, BYTES = 0, 1
# the keys the totals of a scan that writes its reads go by, in the scan's own units (pairs or reads): totals [0], [1]
# and [2] + [3]
WRITE_COUNTER_KEYS = ("written_records", "written_bases", "written_bytes")


def capacity(text_bytes: int, n: int) -> int:
    """What a side's output can never pass: ``GF_RW_CAPACITY``."""
    return int(text_bytes) + 1 + int(n) * TAG_MAX


class GfRwSettings(C.Structure):
    _fields_ = [("umi_source", C.c_int32), ("umi_length", C.c_int32), ("gather", C.c_int32)]


_vp, _i64 = C.c_void_p, C.c_int64


class GfRwSide(C.Structure):
    _fields_ = [("d_text", _vp), ("text_bytes", _i64), ("d_nl_pos", _vp), ("newlines", _i64), ("d_bases", _vp),
                ("d_quals", _vp), ("d_off", _vp), ("d_pre_bases", _vp), ("d_pre_off", _vp), ("d_out_text", _vp),
                ("out_cap", _i64), ("d_out_off", _vp)]


# libgfwrite.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfwrite.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(RW_LIB_PATH, "FASTQ output", "gf_rw_last_error", {
    "gf_rw_workspace_bytes": (_i64, [_i64]),
    "gf_rw_format_device": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "gf_rw_last_error": (C.c_char_p, []),
})


def _address(t, nothing):
    # (records without a base: an empty tensor has no address, and the library wants one with records)
    return (t if t.numel() else nothing).data_ptr()


def format_reads_device(indexer, texts, cuts, finals, n: int, pre=None, umi=None, gather: int = WIDE, stream=None):
    """The first ``n`` records of every side formatted as FASTQ text on the device: (out texts, out offsets, totals).
    ``texts``: per side the uint8 device tensor of the FASTQ text; ``cuts``: per side the ``FastqBatch`` cut from it
    (for its newline index); ``finals``: per side the batch the last preparation step left, the qualities at the
    bases' offsets.  ``pre`` and ``umi``: per side the batch as it stood before the UMI cut and the inline ``Umi`` — the
    tag ``:UMI`` then goes into every name; both None: no tag.  ``out texts``: per side a uint8 device tensor of the
    capacity, of which ``out offsets[side][n]`` bytes are text; ``totals``: the int64[5] device tensor of this call.
    Asynchronous."""
    import torch
    from .umi import SOURCES
    if (pre is None) != (umi is None):
        raise ValueError("format_reads_device takes the pre-cut batches and the Umi together, or neither")
    if umi is not None and not umi.inline:
        raise ValueError("format_reads_device tags with an inline Umi, not %r: the name source's UMI is in the name" % (umi,))
    if not len(texts) == len(cuts) == len(finals) or len(texts) not in (1, 2) or (pre is not None and len(pre) != len(texts)):
        raise ValueError("format_reads_device takes one side or two, the same of everything")
    if umi is not None:
        umi.need_sides(len(texts))
    n = int(n)
    dev = texts[0].device
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    L = lib()
    sides, keep = [], [nothing]
    for k, (text, cut, b) in enumerate(zip(texts, cuts, finals)):
        if b.qual_off is not None:
            raise ValueError("format_reads_device takes the full FASTQ cut: the qualities at the bases' offsets")
        _lib.need_device_tensors("format_reads_device", text, cut.nl_pos, b.bases, b.quals, b.offsets)
        assert text.dtype == torch.uint8 and text.is_contiguous()
        assert cut.nl_pos.dtype == torch.int64 and cut.nl_pos.is_contiguous()
        assert b.bases.dtype == torch.uint8 and b.quals.dtype == torch.uint8 and b.offsets.dtype == torch.int64
        assert b.bases.is_contiguous() and b.quals.is_contiguous() and b.offsets.is_contiguous()
        assert b.offsets.numel() >= n + 1 and int(cut.n_newlines) <= cut.nl_pos.numel()
        cap = capacity(text.numel(), n)
        out_text = torch.empty(cap, dtype=torch.uint8, device=dev)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        side = GfRwSide(text.data_ptr() if text.numel() else None, int(text.numel()),
                        cut.nl_pos.data_ptr() if int(cut.n_newlines) else None, int(cut.n_newlines),
                        _address(b.bases, nothing), _address(b.quals, nothing), b.offsets.data_ptr(), None, None,
                        out_text.data_ptr(), cap, out_off.data_ptr())
        if pre is not None:
            p = pre[k]
            _lib.need_device_tensors("format_reads_device", p.bases, p.offsets)
            assert p.bases.dtype == torch.uint8 and p.offsets.dtype == torch.int64
            assert p.bases.is_contiguous() and p.offsets.is_contiguous() and p.offsets.numel() >= n + 1
            side.d_pre_bases, side.d_pre_off = _address(p.bases, nothing), p.offsets.data_ptr()
        sides.append(side)
        keep += [out_text, out_off]
    settings = GfRwSettings(SOURCES[umi.source] if umi is not None else 0, umi.length if umi is not None else 0, gather)
    ws_bytes = int(L.gf_rw_workspace_bytes(n))
    ws = _lib.workspace(ws_bytes, dev, stream)
    totals = torch.zeros(TOTALS, dtype=torch.int64, device=dev)
    check(L.gf_rw_format_device(indexer._handle(), C.addressof(settings), C.addressof(sides[0]),
                                C.addressof(sides[1]) if len(sides) == 2 else None, n, ws.data_ptr(), ws_bytes,
                                totals.data_ptr(), _lib.stream_handle(dev, stream)))
    for t in keep + [totals]:
        _lib.for_stream(t, stream)
    return keep[1::2], keep[2::2], totals


class WriteResult(NamedTuple):
    """What a ``ReadWriter`` has written: ``records`` in the scan's own units (pairs or reads), the ``bases`` of both
    mates, the ``bytes`` of FASTQ text per file (before compression), and the records ``not_written``."""
    records: int
    bases: int
    bytes: tuple
    not_written: int


def write_totals_counters(totals) -> dict:
    """The three counters of a call's or a scan's totals (a sequence of five integers), under the keys a scan that
    writes its reads reports."""
    t = [int(x) for x in totals]
    return dict(zip(WRITE_COUNTER_KEYS, (t[0], t[1], t[2] + t[3])))


class _FileWriter(threading.Thread):
    """One output file and the thread that writes it, behind a queue of depth 2: the blocks arrive in file order, and
    whoever hands them over waits only when two are already pending.  A name that ends in ``.gz``: every block becomes
    one gzip member, compressed here; concatenated members are a valid gzip file.  ``raw``: the blocks are BGZF members
    already (deflated on the device) and are written as they are, with ``end`` (the end-of-file marker) behind the last."""

    def __init__(self, path: str, level: int, raw: bool = False, end: bytes = b""):
        super().__init__(name="gf-write-" + os.path.basename(path), daemon=True)
        self.path, self.tmp, self.level = path, path + ".tmp", level
        self.gz = path.endswith(".gz") and not raw
        self.end = end
        self.pending: queue.Queue = queue.Queue(maxsize=2)
        self.error: Optional[BaseException] = None
        self.members = 0
        self.f = open(self.tmp, "wb")

    def member(self, data) -> bytes:
        c = zlib.compressobj(self.level, zlib.DEFLATED, 31)   # (31: a gzip header and trailer around the stream)
        return c.compress(data) + c.flush()

    def run(self) -> None:
        while True:
            item = self.pending.get()
            if item is None:
                return
            data, release = item
            try:
                if self.error is None:   # (after a failure the queue is still emptied: nobody waits for ever)
                    self.f.write(self.member(data) if self.gz else data)
                    self.members += 1
            except BaseException as e:   # noqa: BLE001  (kept for the thread that owns the scan)
                self.error = e
            finally:
                if release is not None:
                    release()

    def stop(self) -> None:
        """The thread joined behind everything pending, the file closed."""
        if self.is_alive():
            self.pending.put(None)
            self.join()
        if not self.f.closed:
            try:
                if self.gz and self.members == 0 and self.error is None:
                    self.f.write(self.member(b""))   # (no record at all: still a gzip file)
                if self.end and self.error is None:
                    self.f.write(self.end)
            finally:
                self.f.close()


class ReadWriter:
    """The files a scan writes its cleaned reads to; the caller owns it, as a ``Dedup`` or a ``ReadQc``, and it serves
    one scan.  ``out1``: the file of R1's records (of the reads, single-end); ``out2``: of R2's, needed with pairs and
    refused without.  Written is every record that still has bases behind the last preparation step — for pairs both
    mates must, so the two files stay in step — in file order, as the four FASTQ lines: the name line as the sequencer
    wrote it, the bases and qualities as the steps left them.  ``umi_in_name``: the inline UMI that ``umi`` cuts off
    goes into the name as ``:UMI`` at the end of its first token ("per_read" on pairs: ``:UMI1_UMI2``), the same for
    both mates, so that a later run with ``Umi("name")`` finds it.  ``compress_level``: zlib's, 1 .. 9, for a name that
    ends in ``.gz``; any other name is written plain.  ``deflate``: who compresses — "host" (the default), the host's
    zlib, one gzip member a chunk; "device", libgfdeflate.so (``deflate``): the text is deflated where it was formatted,
    into BGZF members of 65280 bytes of text, and the file ends with the BGZF end-of-file marker, so that bgzip, htslib
    and a later run with ``inflate="device"`` read it member by member.  "device" needs every output name to end in
    ``.gz``, and ``compress_level`` is not used with it: the device encoder has one setting.  The files are written as
    ``name + ".tmp"`` and renamed when the scan ends; a scan that raises leaves neither.  ``ValueError`` for anything
    else, before a file is opened."""

    def __init__(self, out1: str, out2: Optional[str] = None, umi_in_name: bool = False, compress_level: int = 4,
                 deflate: str = "host"):
        for name, v in (("out1", out1),) + ((("out2", out2),) if out2 is not None else ()):
            if not isinstance(v, str) or not v:
                raise ValueError("ReadWriter.%s must be a file name, not %r" % (name, v))
        if not isinstance(umi_in_name, bool):
            raise ValueError("ReadWriter.umi_in_name must be True or False, not %r" % (umi_in_name,))
        if isinstance(compress_level, bool) or not isinstance(compress_level, int) or not 1 <= compress_level <= 9:
            raise ValueError("ReadWriter.compress_level must be 1 .. 9, not %r" % (compress_level,))
        if not isinstance(deflate, str) or deflate not in ("host", "device"):
            raise ValueError("ReadWriter.deflate must be 'host' or 'device', not %r" % (deflate,))
        if deflate == "device":
            for v in (out1, out2):
                if v is not None and not v.endswith(".gz"):
                    raise ValueError("ReadWriter: deflate='device' writes BGZF, and %r does not end in .gz" % (v,))
        if out2 is not None and _same_file(out1, out2):
            raise ValueError("ReadWriter: out1 and out2 are the same file, %r" % (out1,))
        for v in (out1, out2):
            if v is not None and not os.path.isdir(os.path.dirname(os.path.abspath(v))):
                raise ValueError("ReadWriter: the directory of %r does not exist" % (v,))
        self.out1, self.out2, self.umi_in_name, self.compress_level = out1, out2, umi_in_name, compress_level
        self.deflate = deflate
        self._compressed = None if deflate == "host" else [0] * (1 if out2 is None else 2)
        self._writers = None      # the open files' threads, one per side
        self._free = None         # per side the queue of its two pinned staging blocks (None: not yet allocated)
        self._done = False
        self._totals = [0] * TOTALS

    @property
    def outputs(self) -> tuple:
        return (self.out1,) + (() if self.out2 is None else (self.out2,))

    @property
    def compressed_bytes(self) -> Optional[tuple]:
        """Per file the bytes of the members the device deflated (the end-of-file marker not counted); None on the host
        route, where the writer threads compress."""
        return None if self._compressed is None else tuple(self._compressed)

    def need_route(self, inputs: Sequence[str], umi=None, streamed: bool = True) -> "ReadWriter":
        """``ValueError`` for a route this writer cannot serve: ``inputs`` are the FASTQ files of the scan ((R1, R2) or
        (reads,)), ``umi`` its ``Umi`` or None, ``streamed`` whether it has ``chunk_bytes``.  Opens nothing."""
        if not streamed:
            raise ValueError("write_reads needs chunk_bytes: the whole-file routes have dropped the device text by the "
                             "time the records are ready")
        if len(inputs) == 2 and self.out2 is None:
            raise ValueError("write_reads: paired-end input needs ReadWriter.out2")
        if len(inputs) == 1 and self.out2 is not None:
            raise ValueError("write_reads: single-end input takes no ReadWriter.out2")
        for o in self.outputs:
            for i in inputs:
                if _same_file(o, i):
                    raise ValueError("write_reads: the output %r is one of the inputs" % (o,))
        if self.umi_in_name and (umi is None or not umi.inline):
            raise ValueError("write_reads: umi_in_name needs umi with an inline source (read1, read2 or per_read), not %r"
                             % (umi,))
        if self._done or self._writers is not None:
            raise ValueError("write_reads: this ReadWriter has served a scan; a second one needs its own")
        return self

    # ---- the files

    def open(self, sides: int) -> None:
        """The ``.tmp`` files opened and their threads started; a file that cannot be opened leaves none."""
        if self._done or self._writers is not None:
            raise ValueError("write_reads: this ReadWriter has served a scan; a second one needs its own")
        if sides != len(self.outputs):
            raise ValueError("write_reads: %d output files for %d sides" % (len(self.outputs), sides))
        self._writers = []
        try:
            device = {}
            if self.deflate == "device":
                from .deflate import EOF_MARKER
                device = dict(raw=True, end=EOF_MARKER)
            for path in self.outputs:
                self._writers.append(_FileWriter(path, self.compress_level, **device))
            for w in self._writers:
                w.start()
        except BaseException:
            self.abort()
            raise
        self._free = [None] * sides

    def hand_over(self, side: int, data, release=None) -> None:
        """``data`` (anything with the buffer protocol) queued for the file of ``side``; ``release()`` is called by the
        writer thread once the block is written.  Raises what that thread met earlier."""
        self._raise_writer_error()
        self._writers[side].pending.put((data, release))

    def _raise_writer_error(self) -> None:
        for w in self._writers or ():
            if w.error is not None:
                raise w.error

    def finish(self) -> None:
        """Everything pending written, the files closed and renamed to their names.  A writer's failure is raised here
        at the latest, and then no file is left."""
        if self._writers is None:
            raise ValueError("write_reads: finish without open")
        try:
            for w in self._writers:
                w.stop()
            self._raise_writer_error()
            for w in self._writers:
                os.replace(w.tmp, w.path)
        except BaseException:
            self.abort()
            raise
        self._writers, self._free, self._done = None, None, True

    def abort(self) -> None:
        """The threads joined, the temporaries unlinked."""
        for w in self._writers or ():
            try:
                w.stop()
            except OSError:
                pass
            try:
                os.unlink(w.tmp)
            except FileNotFoundError:
                pass
        self._writers, self._free, self._done = None, None, True

    # ---- a chunk

    def format_chunk(self, indexer, texts, cuts, finals, m: int, pre=None, umi=None):
        """The format call of a chunk's first ``m`` records queued behind the last preparation step: what ``collect``
        takes.  ``pre``: the batches ahead of the UMI cut, used (with ``umi``) only with ``umi_in_name``."""
        tag = dict(pre=[b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in pre], umi=umi) \
            if self.umi_in_name else {}
        formatted = format_reads_device(indexer, texts, cuts,
                                        [b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in finals], m, **tag)
        if self.deflate == "device":
            # the deflate queued behind the format call, on its output: the text's length stays on the device
            from .deflate import deflate_device
            out_texts, out_offs, totals = formatted
            return formatted + ([deflate_device(text, off[m:m + 1]) for text, off in zip(out_texts, out_offs)],)
        return formatted

    def _staging(self, side: int, nbytes: int):
        """One of the side's two pinned staging blocks, of at least ``nbytes``: waits while both are with the writer."""
        import torch
        if self._free[side] is None:
            self._free[side] = queue.Queue()
            for _ in range(2):
                self._free[side].put(None)
        while True:
            try:
                block = self._free[side].get(timeout=0.5)
                break
            except queue.Empty:   # (a writer that died holds no block back, but say what it met)
                self._raise_writer_error()
        if block is None or block.numel() < nbytes:
            block = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, pin_memory=True)
        return block

    def collect(self, formatted) -> dict:
        """Behind the chunk's read-back: the totals of ``format_chunk``'s call read, the text of every side copied into
        a staging block and handed to its file's thread.  Returns the chunk's three counters."""
        out_texts, _, totals = formatted[:3]
        if self.deflate == "device":
            import torch
            from .deflate import TOTALS as DEFLATE_TOTALS
            deflated = formatted[3]
            both = [int(x) for x in torch.cat([totals] + [d[2] for d in deflated]).cpu().tolist()]   # (one read-back)
            t = both[:TOTALS]
            packed = [both[TOTALS + DEFLATE_TOTALS * k:TOTALS + DEFLATE_TOTALS * (k + 1)] for k in range(len(deflated))]
        else:
            t = [int(x) for x in totals.cpu().tolist()]
        for side, text in enumerate(out_texts):
            nbytes = t[2 + side]
            if nbytes > text.numel():
                raise _lib.GfError(_lib.GF_ERR_CAPACITY, "write_reads: a chunk's records are longer than its text")
            if nbytes == 0:
                continue
            if self.deflate == "device":   # (the members of this side's text, as they are)
                text, members, text_bytes, nbytes = deflated[side][0], packed[side][0], packed[side][1], packed[side][2]
                if text_bytes != t[2 + side] or nbytes > text.numel() or members != -(-text_bytes // 65280):
                    raise _lib.GfError(_lib.GF_ERR_CAPACITY, "write_reads: the deflate's totals do not fit its text")
                self._compressed[side] += nbytes
            block = self._staging(side, nbytes)
            block[:nbytes].copy_(text[:nbytes])
            free = self._free[side]
            self.hand_over(side, block[:nbytes].numpy(), lambda free=free, block=block: free.put(block))
        for k in range(TOTALS):
            self._totals[k] += t[k]
        return write_totals_counters(t)

    def result(self) -> WriteResult:
        t = self._totals
        return WriteResult(t[0], t[1], (t[2],) + (() if self.out2 is None else (t[3],)), t[4])

    def __repr__(self) -> str:
        return "ReadWriter(out1=%r, out2=%r, umi_in_name=%r, compress_level=%d)%s" % (
            self.out1, self.out2, self.umi_in_name, self.compress_level,
            "" if self.deflate == "host" else "[deflate=%r]" % (self.deflate,))


def _same_file(a: str, b: str) -> bool:
    if os.path.realpath(a) == os.path.realpath(b):
        return True
    try:
        return os.path.samefile(a, b)
    except OSError:
        return False


def need_read_writer(x) -> Optional[ReadWriter]:
    """``x`` when it is None or a ``ReadWriter``; ``ValueError`` for anything else."""
    if x is None or isinstance(x, ReadWriter):
        return x
    raise ValueError("write_reads must be None or a ReadWriter, not %r" % (x,))
