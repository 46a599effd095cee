"""The gene slices of a reference FASTA, cut out on the device while the file is read in chunks: libgfrefcut.so
(include/gf_ref_cut.h) and the host side that drives it.

``scan.read_contigs`` holds the whole, gunzipped FASTA and two or three copies of it before ``Indexer.make_index`` cuts
out the few Mbp it needs.  ``cut_gene_slices`` gives the same slices — exactly what ``FastaReader.read_all`` +
``resolve_gene_slice`` give, quirks included — with the text crossing the host a chunk at a time:

    byte source (the file, gunzipped as it is read)  --readinto, an upload thread-->  pinned staging block
    --H2D, copy stream-->  device text buffer (behind the carried-over unfinished header of the previous chunk)  -->
    gf_rc_index_device (records, names, kept counts)  -->  one small read-back  -->  ``CutPlan`` (which ranges of which
    records are wanted)  -->  gf_rc_gather_device  -->  the wanted bytes, upper-cased, back to the host.

The chunk loop — staging blocks, upload thread, text buffers, carry — is ``chunk_stream.ChunkStream``, the one the streamed
FASTQ scans run on.  ``CutPlan`` is pure Python and needs no GPU.  libgfrefcut.so is a library of its own next to libgfmatch.so
(genefuserust_amd/scan_csrc/); it is loaded after ``_lib.lib()``, whose pinned allocator the staging blocks come from.
No CPU fallback: without the libraries and a GPU every device call raises.
"""
from __future__ import annotations

import bisect
import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import GF_ERR_CAPACITY, GfError
from .chunk_stream import CARRY_MAX, ChunkStream, checked_chunk_bytes, whole_read_sizes
from .fastq import FastqByteStream
from .indexer import Fusion

RC_LIB_PATH = os.path.join(_lib._HERE, "libgfrefcut.so")

_vp, _i64 = C.c_void_p, C.c_int64
# libgfrefcut.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfrefcut.so links against.
lib, check = _lib.companion(RC_LIB_PATH, "reference cut", "gf_rc_last_error", {
    "gf_rc_tile_bytes": (_i64, []),
    "gf_rc_tiles": (_i64, [_i64]),
    "gf_rc_workspace_bytes": (_i64, [_i64]),
    "gf_rc_index_device": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "gf_rc_gather_device": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "gf_rc_copy_from_host_device": (C.c_int, [_vp, _vp, _i64, _vp]),
    "gf_rc_last_error": (C.c_char_p, []),
})


def tile_bytes() -> int:
    """Bytes of text per tile of the kernels (``gf_rc_tile_bytes``)."""
    return int(lib().gf_rc_tile_bytes())


# ---- the two device calls -----------------------------------------------------------------------------------------

class ChunkRecords(NamedTuple):
    """The read-back of ``RefIndex.download``: ``n`` records started in the chunk and, for record k = 1 .. n at index
    k - 1, ``gt_pos`` / ``gt_rank`` / ``name_end`` / ``seq_rank`` (include/gf_ref_cut.h) and ``names``; ``kept`` kept
    bytes in the chunk, ``unfinished`` where an unfinished header begins (-1: none)."""
    n: int
    kept: int
    unfinished: int
    gt_pos: np.ndarray
    gt_rank: np.ndarray
    name_end: np.ndarray
    seq_rank: np.ndarray
    names: List[bytes]


class RefIndex(NamedTuple):
    """What gf_rc_index_device leaves in HBM.  ``block`` (int64) holds, back to back, the totals [8], ``gt_pos``,
    ``gt_rank``, ``name_end``, ``seq_rank`` [cap_records each], the name offsets [cap_records + 1] and the names'
    bytes, so that one copy brings all of it to the host; ``tile_kept`` int64[tiles + 1] stays on the device."""
    block: "object"
    tile_kept: "object"
    cap_records: int
    names_cap: int

    def part(self, k: int):
        """Part k of ``block``: 0 totals, 1 gt_pos, 2 gt_rank, 3 name_end, 4 seq_rank, 5 name offsets, 6 names."""
        cap = self.cap_records
        starts = [0, 8, 8 + cap, 8 + 2 * cap, 8 + 3 * cap, 8 + 4 * cap, 8 + 5 * cap + 1, self.block.numel()]
        return self.block[starts[k]:starts[k + 1]]

    def download(self) -> ChunkRecords:
        """Synchronises; one copy.  ``GfError(GF_ERR_CAPACITY)`` when ``cap_records`` or ``names_cap`` was too small
        (``needed`` on the error says what the call needs: (records, name bytes))."""
        host = self.block.cpu().numpy()
        cap = self.cap_records
        n, kept, over, unfinished, name_bytes = (int(x) for x in host[:5])
        if over:
            e = GfError(GF_ERR_CAPACITY, "the chunk has %d records and %d bytes of names; cap_records is %d, names_cap %d"
                        % (n, name_bytes, cap, self.names_cap))
            e.needed = (n, name_bytes if not over & 1 else None)
            raise e
        arr = [host[8 + k * cap:8 + k * cap + n] for k in range(4)]
        off = host[8 + 4 * cap:8 + 4 * cap + n + 1]
        buf = host[8 + 5 * cap + 1:].view(np.uint8)[:name_bytes].tobytes()
        return ChunkRecords(n, kept, unfinished, *arr, [buf[off[k]:off[k + 1]] for k in range(n)])


def _device_text(text, what: str):
    import torch
    _lib.need_device_tensors(what, text)
    assert text.dtype == torch.uint8 and text.is_contiguous()


def ref_index_device(text, cap_records: int = 1024, names_cap: int = 1 << 16, stream=None) -> RefIndex:
    """The records of a chunk of FASTA text (uint8 device tensor, any alignment), asynchronously: gf_rc_index_device."""
    import torch
    _device_text(text, "ref_index_device")
    L = lib()
    dev = text.device
    n = text.numel()
    cap_records, names_cap = int(cap_records), int(names_cap)
    ws_bytes = int(L.gf_rc_workspace_bytes(n))
    ws = _lib.workspace(ws_bytes, dev, stream)
    tile_kept = torch.empty(int(L.gf_rc_tiles(n)) + 1, dtype=torch.int64, device=dev)
    ix = RefIndex(torch.empty(8 + 5 * cap_records + 1 + (names_cap + 7) // 8, dtype=torch.int64, device=dev), tile_kept,
                  cap_records, names_cap)
    totals, gt_pos, gt_rank, name_end, seq_rank, name_off, names = (ix.part(k) for k in range(7))
    check(L.gf_rc_index_device(text.data_ptr() if n else None, n, cap_records, ws.data_ptr(), ws_bytes,
                               gt_pos.data_ptr(), gt_rank.data_ptr(), name_end.data_ptr(), seq_rank.data_ptr(),
                               name_off.data_ptr(), names.data_ptr() if names_cap else None, names_cap,
                               tile_kept.data_ptr(), totals.data_ptr(), _lib.stream_handle(dev, stream)))
    return ix


def ref_gather_device(text, index: RefIndex, n_records: int, intervals, out_bytes: int, carried_kept: int = 0,
                      out=None, stream=None):
    """The kept bytes of ``intervals`` — rows (record ordinal, start, end, offset in the output), disjoint, sorted by
    record and start — upper-cased, into a uint8 device tensor of ``out_bytes`` (``out``: one to write into),
    asynchronously: gf_rc_gather_device.  ``text`` is the text of the index call or a front part of it."""
    import torch
    _device_text(text, "ref_gather_device")
    dev = text.device
    iv = np.ascontiguousarray(np.asarray(intervals, dtype=np.int64).reshape(-1, 4))
    d_iv = _lib.for_stream(torch.from_numpy(iv).to(dev), stream)
    if out is None:
        out = torch.empty(max(int(out_bytes), 1), dtype=torch.uint8, device=dev)
    n = text.numel()
    check(lib().gf_rc_gather_device(text.data_ptr() if n else None, n, index.part(1).data_ptr(),
                                    index.part(4).data_ptr(), int(n_records), index.tile_kept.data_ptr(),
                                    int(carried_kept), d_iv.data_ptr() if iv.shape[0] else None, iv.shape[0],
                                    out.data_ptr(), int(out_bytes), _lib.stream_handle(dev, stream)))
    return out


# ---- the planning: which ranges of which records are wanted (no GPU) ------------------------------------------------

def candidate_names(chr_: str) -> List[str]:
    """The contig names ``resolve_gene_slice`` tries for a gene's chromosome, in its order of precedence (indexer.rs:
    137-147): the name, "chr" + name, the name with every "chr" struck."""
    out: List[str] = []
    for c in (chr_, "chr" + chr_, chr_.replace("chr", "")):
        if c not in out:
            out.append(c)
    return out


def merge_ranges(ranges: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """Half-open ranges -> disjoint ones in ascending order: overlapping and touching ranges become one, empty ranges
    and those that no contig can hold (negative start, end before start) none."""
    out: List[List[int]] = []
    for s, e in sorted((s, e) for s, e in ranges if 0 <= s < e):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [(s, e) for s, e in out]


class Contig:
    """One record of the FASTA whose name some gene asks for: how many sequence bytes it has had so far (``length``) and
    the bytes of its wanted ranges (``intervals``, disjoint and ascending), filled front to back as the chunks go by."""

    def __init__(self, name: str, intervals: List[Tuple[int, int]]):
        self.name = name
        self.length = 0
        self.intervals = intervals
        self._starts = [s for s, _ in intervals]
        self.data = [bytearray() for _ in intervals]

    def wanted(self, lo: int, hi: int) -> List[Tuple[int, int, int]]:
        """(interval number, start, end) of the parts of the wanted ranges inside positions [lo, hi)."""
        out = []
        for i in range(max(bisect.bisect_right(self._starts, lo) - 1, 0), len(self.intervals)):
            s, e = self.intervals[i]
            if s >= hi:
                break
            if max(s, lo) < min(e, hi):
                out.append((i, max(s, lo), min(e, hi)))
        return out

    def put(self, i: int, start: int, data: bytes) -> None:
        """The bytes at positions start .. of interval i: they arrive in order."""
        assert start == self.intervals[i][0] + len(self.data[i])
        self.data[i] += data

    def cut(self, start: int, end: int) -> bytes:
        """Positions [start, end) (inside the contig) out of the interval that holds them."""
        if start == end:
            return b""
        i = bisect.bisect_right(self._starts, start) - 1
        s = self.intervals[i][0]
        return bytes(self.data[i][start - s:end - s])


class CutPlan:
    """What a pass over the FASTA has to bring for the genes of ``fusion_lists`` (lists of ``Fusion``, one per CSV): per
    contig name any gene may resolve to, the merged ranges of the genes that may.  The pass reports each record as it
    starts (``start_record``), feeds the ``Contig`` it gets, and at the end ``finish`` resolves every gene the way
    ``resolve_gene_slice`` does on the whole map of contigs."""

    def __init__(self, fusion_lists: Sequence[Sequence[Fusion]]):
        self.fusion_lists = [list(fl) for fl in fusion_lists]
        ranges: Dict[str, List[Tuple[int, int]]] = {}
        for fl in self.fusion_lists:
            for f in fl:
                g = f.m_gene
                for name in candidate_names(g.m_chr):
                    ranges.setdefault(name, []).append((g.m_start, g.m_end))
        self.intervals = {name: merge_ranges(r) for name, r in ranges.items()}
        self.seen: Dict[str, Contig] = {}

    def start_record(self, name: str) -> Optional[Contig]:
        """A record named ``name`` starts: its ``Contig`` when a gene may want it, else None.  A name that comes again
        replaces the earlier record (the map of contigs keeps the last)."""
        if name not in self.intervals:
            return None
        c = self.seen[name] = Contig(name, self.intervals[name])
        return c

    def finish(self) -> List[List[Optional[bytes]]]:
        """Per fusion list, per gene: its slice, or None when none of its names occurred.  Raises ``IndexError`` with
        ``resolve_gene_slice``'s message for a range outside the contig chosen — a name of lower precedence is not
        looked at, in range or not."""
        out = []
        for fl in self.fusion_lists:
            slices: List[Optional[bytes]] = []
            for f in fl:
                g = f.m_gene
                c = next((self.seen[n] for n in candidate_names(g.m_chr) if n in self.seen), None)
                if c is None:
                    slices.append(None)
                    continue
                if not (0 <= g.m_start <= g.m_end <= c.length):
                    raise IndexError("gene %s: range %d..%d outside contig %s (len %d)"
                                     % (g.m_name, g.m_start, g.m_end, c.name, c.length))
                slices.append(c.cut(g.m_start, g.m_end))
            out.append(slices)
        return out


def plan_chunk(plan: CutPlan, open_rec: Optional[Contig], rec: ChunkRecords, text_bytes: int, final: bool):
    """One chunk's records against the plan.  ``open_rec``: the ``Contig`` the chunk starts in (None: a record nobody
    wants, or the bytes in front of the first record); ``final``: the file ends with this chunk.  Returns (records to
    know of, bytes of text to gather from, interval rows for gf_rc_gather_device, [(contig, interval number, start,
    offset in the output, length)] to file the gathered bytes by, the contig per ordinal, kept bytes per ordinal).
    An unfinished header at the end of a chunk that is not the last is left out: it comes again, whole, in front of the
    next chunk."""
    n, kept, nbytes = rec.n, rec.kept, text_bytes
    if rec.unfinished >= 0 and not final:
        n, kept, nbytes = n - 1, int(rec.gt_rank[n - 1]), rec.unfinished
    recs: List[Optional[Contig]] = [open_rec]
    for k in range(n):
        # (a '>' that ends the file starts nothing: read_until returns no bytes there)
        last_empty = final and k == rec.n - 1 and rec.name_end[k] < 0 and not rec.names[k]
        recs.append(None if last_empty else plan.start_record(rec.names[k].decode("latin-1")))
    ends = [int(x) for x in rec.gt_rank[:n]] + [kept]
    starts = [0] + [int(x) for x in rec.seq_rank[:n]]
    kept_of = [e - s for s, e in zip(starts, ends)]
    rows, filing, off = [], [], 0
    for k, c in enumerate(recs):
        if c is None:
            continue
        lo = c.length   # (0 for a record that starts in this chunk)
        for i, s, e in c.wanted(lo, lo + kept_of[k]):
            rows.append((k, s, e, off))
            filing.append((c, i, s, off, e - s))
            off += e - s
    return n, nbytes, rows, filing, recs, kept_of


class CutPass:
    """The host's state between the chunks of one pass: the plan and the record the next chunk starts in."""

    def __init__(self, plan: CutPlan):
        self.plan = plan
        self.open_rec: Optional[Contig] = None

    def chunk(self, rec: ChunkRecords, text_bytes: int, final: bool, gather) -> int:
        """One chunk, its records read back: plans it, has ``gather(records, bytes of text, interval rows, bytes of
        output, carried_kept) -> bytes`` bring the wanted bytes, files them and counts the records' lengths on.
        Returns how many bytes of the text are done with; the rest is carried to the front of the next chunk."""
        n, nbytes, rows, filing, recs, kept_of = plan_chunk(self.plan, self.open_rec, rec, text_bytes, final)
        if rows:
            total = rows[-1][3] + rows[-1][2] - rows[-1][1]
            got = gather(n, nbytes, rows, total, self.open_rec.length if self.open_rec is not None else 0)
            for c, i, s, off, ln in filing:
                c.put(i, s, got[off:off + ln])
        for c, k in zip(recs, kept_of):
            if c is not None:
                c.length += k
        self.open_rec = recs[-1]
        return nbytes


# ---- the pass over the file ---------------------------------------------------------------------------------------

def _index_with_room(text, caps: dict) -> Tuple[RefIndex, ChunkRecords]:
    """``ref_index_device`` + its read-back, once more with the room the first call asked for when it was too small
    (``caps`` keeps what was needed for the chunks that follow)."""
    while True:
        ix = ref_index_device(text, **caps)
        try:
            return ix, ix.download()
        except GfError as e:
            if e.code != GF_ERR_CAPACITY:
                raise
            n, name_bytes = e.needed
            caps["cap_records"] = max(caps["cap_records"], n)
            if name_bytes is not None:   # (at least twice the room: a long header grows from chunk to chunk)
                caps["names_cap"] = max(2 * caps["names_cap"], name_bytes)


def cut_gene_slices(ref_file: str, fusion_lists: Sequence[Sequence[Fusion]], chunk_bytes: int,
                    device: int = -1, inflate: str = "host") -> List[List[Optional[bytes]]]:
    """Per fusion list, per gene, what ``resolve_gene_slice(read_contigs(ref_file), gene)`` gives — one pass over the
    FASTA serves all lists — with the file read, gunzipped and uploaded in chunks of ``chunk_bytes`` of plain text
    while the device indexes and gathers the previous chunk.  The host holds two pinned staging blocks of
    ``chunk_bytes`` and the wanted bytes, the device two text buffers.  ``device``: -1 is the current one.  Raises as
    the host reader does: ``IsADirectoryError``, ``ValueError`` for an empty file, ``IndexError`` for a range outside
    its contig; ``GfError(GF_ERR_CAPACITY)`` for a record name of more than 1 MiB.  ``inflate``: "host" gunzips a ``.gz``
    file on the host; "auto" / "device" send a BGZF file's compressed bytes to the device (bgzf.py, ``scan.open_index``)."""
    import torch
    ref_file = str(ref_file)
    chunk_bytes = checked_chunk_bytes(chunk_bytes)
    if os.path.isdir(ref_file):
        raise IsADirectoryError("There is a problem with the provided fasta file: '%s' is a directory NOT a file..."
                                % ref_file)
    plan = CutPlan(fusion_lists)
    dev = torch.device("cuda", torch.cuda.current_device() if device < 0 else device)
    caps = dict(cap_records=1024, names_cap=1 << 16)
    state = CutPass(plan)

    def copy(ptr: int, dst: int, n: int, stream: int) -> None:
        check(lib().gf_rc_copy_from_host_device(ptr, dst, n, stream))

    def cut(texts, final):
        text, = texts
        if text.numel() == 0:   # (the first chunk: the chunk that holds a file's last byte is its last)
            raise ValueError("empty fasta file: %s" % ref_file)
        ix, rec = _index_with_room(text, caps)
        nbytes = state.chunk(rec, text.numel(), final[0], lambda n, nbytes, rows, total, carried: (
            ref_gather_device(text[:nbytes], ix, n, rows, total, carried).cpu().numpy().tobytes()))
        if text.numel() - nbytes > CARRY_MAX:
            raise GfError(GF_ERR_CAPACITY, "%s: a record name of more than %d bytes" % (ref_file, CARRY_MAX))
        return [nbytes], [True], None

    from .bgzf import open_source
    with open_source(ref_file, inflate, lambda: FastqByteStream(ref_file, ref_file.endswith(".gz"))) as source:
        for _ in ChunkStream([source], chunk_bytes, dev, copy, whole_read_sizes).run(cut):
            pass
    return plan.finish()
