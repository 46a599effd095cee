"""The names of the reads a scan matched, gathered on the device: ``gf_hn_names_device`` of libgfnames.so
(include/gf_hit_names.h); and, for the HTML report, their whole FASTQ records: ``gf_hn_records_device``
(include/gf_hit_records.h).

A ``ReadMatch`` carries the name of the read it was found on.  The whole-file scans cut it from the host copy of the
FASTQ text (``fastq.record_lines``); here the name lines of the hit records are copied out of the text while it is still
in HBM, in one asynchronous call, so that a streamed scan can drop a chunk's text as soon as the chunk is scanned
(scan_stream.py).  libgfnames.so is a library of its own on top of libgfmatch.so's public C ABI
(genefuserust_amd/scan_csrc/); it is loaded after ``_lib.lib()`` so that both refer to the one libgfmatch.so of this
tree.  No CPU fallback: without the libraries and a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, NamedTuple, Optional, Tuple

from . import _lib
from ._lib import GF_ERR_CAPACITY, GfError
from .indexer import Indexer
from .read_pair import PairScan

HN_LIB_PATH = os.path.join(_lib._HERE, "libgfnames.so")

_vp, _i64 = C.c_void_p, C.c_int64
_GATHER = (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp,
                     _vp])
# libgfnames.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfnames.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(HN_LIB_PATH, "hit-name gather", "gf_hn_last_error", {
    "gf_hn_workspace_bytes": (_i64, [_i64]),
    "gf_hn_names_device": _GATHER,
    "gf_hn_records_workspace_bytes": (_i64, [_i64]),
    "gf_hn_records_device": _GATHER,
    "gf_hn_last_error": (C.c_char_p, []),
})


class HitNames(NamedTuple):
    """What gf_hn_names_device leaves in HBM: ``names`` uint8[names_cap] (the names back to back), ``offsets``
    int64[hits_cap + 1], ``totals`` int64[4] (names, their bytes, overflow bit, records without a name line)."""
    names: "object"
    offsets: "object"
    totals: "object"

    def download(self) -> List[bytes]:
        """Synchronises.  The names in record order; ``GfError(GF_ERR_CAPACITY)`` when ``names_cap`` was too small
        (the message says how many bytes are needed)."""
        n, nbytes, over, _ = (int(x) for x in self.totals.cpu())
        if over:
            raise GfError(GF_ERR_CAPACITY, "the names take %d bytes, names_cap is %d" % (nbytes, self.names.numel()))
        off = self.offsets[:n + 1].cpu().numpy()
        buf = self.names[:nbytes].cpu().numpy().tobytes()
        return [buf[off[k]:off[k + 1]] for k in range(n)]


def _gather(what: str, fn, ws_fn, per_record: int, indexer, scan, l_text, l_batch, r_text, r_batch, pair_id_base, cap,
            stream):
    """What both gathers share around their call: the checks of the tensors, the outputs — (bytes, offsets, totals),
    ``per_record`` offsets per record capacity plus one — and the workspace.  ``cap`` None: the bytes ``what`` takes
    by default for the record capacity."""
    import torch
    tensors = [scan.hits, scan.totals, l_text, l_batch.nl_pos] + ([] if r_text is None else [r_text, r_batch.nl_pos])
    _lib.need_device_tensors(what, *tensors)
    assert l_text.dtype == torch.uint8 and l_text.is_contiguous() and l_batch.nl_pos.dtype == torch.int64
    assert l_batch.nl_pos.is_contiguous() and l_batch.nl_pos.numel() >= l_batch.n_newlines
    if r_text is not None:
        assert r_text.dtype == torch.uint8 and r_text.is_contiguous() and r_batch.nl_pos.dtype == torch.int64
        assert r_batch.nl_pos.is_contiguous() and r_batch.nl_pos.numel() >= r_batch.n_newlines
    dev = l_text.device
    hits_cap = int(scan.hits.shape[0])
    cap = int(cap(hits_cap) if callable(cap) else cap)
    ws_bytes = int(ws_fn(hits_cap))
    ws = _lib.workspace(ws_bytes, dev, stream)
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    offsets = torch.empty(per_record * hits_cap + 1, dtype=torch.int64, device=dev)
    totals = torch.zeros(4, dtype=torch.int64, device=dev)
    right = (None, 0, None, 0) if r_text is None else (r_text.data_ptr(), r_text.numel(), r_batch.nl_pos.data_ptr(),
                                                       int(r_batch.n_newlines))
    check(fn(indexer._handle(), scan.hits.data_ptr(), scan.totals.data_ptr(), hits_cap, int(pair_id_base),
             l_text.data_ptr(), l_text.numel(), l_batch.nl_pos.data_ptr(), int(l_batch.n_newlines), *right, ws.data_ptr(),
             ws_bytes, out.data_ptr(), cap, offsets.data_ptr(), totals.data_ptr(), _lib.stream_handle(dev, stream)))
    return out, offsets, totals


def hit_names_device(indexer: Indexer, scan: PairScan, l_text, l_batch, r_text=None, r_batch=None,
                     pair_id_base: int = 0, names_cap: Optional[int] = None, stream=None) -> HitNames:
    """The name lines of the records of ``scan``, asynchronously.  ``l_text`` (uint8 device tensor) is the FASTQ text
    the scanned records were cut from and ``l_batch`` its ``FastqBatch`` (for the newline index); ``r_text`` /
    ``r_batch`` the same for R2, ``None`` for single-end input.  ``pair_id_base`` is what the scan was given: record k
    names FASTQ record ``pair_id - pair_id_base`` — of R2 when its ``source`` is 2, else of R1 — and gets what
    ``fastq.record_lines(batch, text, i)[0]`` returns.  ``names_cap``: bytes for the names (default: 64 per record
    capacity; ``totals`` says when that was too small, and how much is needed)."""
    L = lib()
    return HitNames(*_gather("hit_names_device", L.gf_hn_names_device, L.gf_hn_workspace_bytes, 1, indexer, scan, l_text,
                             l_batch, r_text, r_batch, pair_id_base,
                             (lambda hits_cap: 64 * hits_cap) if names_cap is None else names_cap, stream))


class HitRecords(NamedTuple):
    """What gf_hn_records_device leaves in HBM: ``records`` uint8[records_cap] (the spans back to back), ``offsets``
    int64[sides * hits_cap + 1], ``totals`` int64[4] (spans, their bytes, overflow bit, spans without a record);
    ``sides``: the spans per hit record, 2 for paired input, else 1."""
    records: "object"
    offsets: "object"
    totals: "object"
    sides: int

    def download(self) -> List[List[Tuple[bytes, bytes, bytes, bytes]]]:
        """Synchronises.  Per hit record, in record order, the (name, sequence, strand, quality) of each side — what
        ``fastq.record_lines`` gives for it: the reference's reader strips only the newline.
        ``GfError(GF_ERR_CAPACITY)`` when ``records_cap`` was too small (the message says how many bytes are needed)."""
        spans, nbytes, over, _ = (int(x) for x in self.totals.cpu())
        if over:
            raise GfError(GF_ERR_CAPACITY, "the records take %d bytes, records_cap is %d" % (nbytes, self.records.numel()))
        off = self.offsets[:spans + 1].cpu().numpy()
        buf = self.records[:nbytes].cpu().numpy().tobytes()
        lines = [tuple((buf[off[j]:off[j + 1]].split(b"\n") + [b""] * 3)[:4]) for j in range(spans)]
        return [lines[j:j + self.sides] for j in range(0, spans, self.sides)]


def hit_records_device(indexer: Indexer, scan: PairScan, l_text, l_batch, r_text=None, r_batch=None,
                       pair_id_base: int = 0, records_cap: Optional[int] = None, stream=None) -> HitRecords:
    """The whole FASTQ records of the records of ``scan``, asynchronously: ``ReadMatch.m_original_reads`` of the
    reference, for the HTML report.  Arguments as for ``hit_names_device``.  Record k gets FASTQ record
    ``pair_id - pair_id_base`` of R1 and, with ``r_text``, of R2 — both, whatever its ``source`` — each what
    ``fastq.record_lines(batch, text, i)`` returns.  ``records_cap``: bytes for the records (default: 1024 per record
    capacity and side, at most the bytes of the texts; ``totals`` says when that was too small, and how much is
    needed)."""
    L = lib()
    sides = 1 if r_text is None else 2
    text_bytes = l_text.numel() + (0 if r_text is None else r_text.numel())

    def default_cap(hits_cap: int) -> int:
        return min(1024 * sides * hits_cap, text_bytes)
    return HitRecords(*_gather("hit_records_device", L.gf_hn_records_device, L.gf_hn_records_workspace_bytes, sides,
                               indexer, scan, l_text, l_batch, r_text, r_batch, pair_id_base,
                               default_cap if records_cap is None else records_cap, stream), sides)
