"""Read QC on the device, opt-in: the per-cycle quality and base-content tables and the insert-size histogram of the
records, ``gf_qc_stats_device`` and ``gf_qc_insert_device`` of libgfqc.so (include/gf_read_qc.h).

With the read filter and the adapter trimming on the device a pipeline needs no fastp in front of a scan, and so it has
no QC report to accept or reject a sample on.  Here the numbers of that report are taken while the records sit in HBM:
before the trimming and the filter, and behind them.  Both passes only read; every number is an exact integer sum, and
reads, bases, Q20 / Q30 rates, GC content, mean lengths and the curves are derived from the tables on the host
(``QcResult``, ``report_json``).  A feature outside the reference, off unless a ``ReadQc`` is handed to a route.
libgfqc.so is a library of its own on top of libgfmatch.so's public C ABI (genefuserust_amd/scan_csrc/).  No CPU
fallback: without the libraries and a GPU every device call raises.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib

QC_LIB_PATH = os.path.join(_lib._HERE, "libgfqc.so")

CYCLES, COLUMNS = 512, 8
SIDE_WORDS = (CYCLES + 1) + (CYCLES + 1) * COLUMNS   # 4617: length_hist[513], then cycle[513][8]
INSERT_WORDS, INSERT_UNMEASURED, INSERT_MIN = 1026, 1025, 30
COL_A, COL_C, COL_G, COL_T, COL_N, COL_QUAL_SUM, COL_Q20, COL_Q30 = range(8)
STAGES = ("before", "after")

_vp, _i64 = C.c_void_p, C.c_int64
# libgfqc.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfqc.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(QC_LIB_PATH, "read QC", "gf_qc_last_error", {
    "gf_qc_stats_device": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "gf_qc_insert_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "gf_qc_last_error": (C.c_char_p, []),
})


def _need_batch(what: str, b, n: int) -> None:
    import torch
    _lib.need_device_tensors(what, b.bases, b.quals, b.offsets)
    assert b.bases.dtype == torch.uint8 and b.quals.dtype == torch.uint8 and b.offsets.dtype == torch.int64
    assert b.bases.is_contiguous() and b.quals.is_contiguous() and b.offsets.is_contiguous()
    assert int(b.n_records) == n and b.offsets.numel() >= n + 1


def _need_table(what: str, table, words: int) -> None:
    import torch
    _lib.need_device_tensors(what, table)
    assert table.dtype == torch.int64 and table.is_contiguous() and table.numel() == words


def _address(t, nothing):
    # (records without a base: an empty tensor has no address, and the library wants one with records)
    return (t if t.numel() else nothing).data_ptr()


def qc_stats_device(indexer, batch, table, stream=None) -> None:
    """The records of ``batch`` (a ``FastqBatch`` of the full cut: the qualities at the bases' offsets) ADDED into
    ``table``, an int64[SIDE_WORDS] device tensor that the caller zeroed once: asynchronously, in one call.
    ``ValueError`` for a lean cut."""
    import torch
    if batch.qual_off is not None:
        raise ValueError("qc_stats_device takes the full FASTQ cut: the qualities at the bases' offsets")
    n = int(batch.n_records)
    _need_batch("qc_stats_device", batch, n)
    _need_table("qc_stats_device", table, SIDE_WORDS)
    assert batch.quals.numel() >= batch.bases.numel()
    dev = batch.bases.device
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    check(lib().gf_qc_stats_device(indexer._handle(), _address(batch.bases, nothing), _address(batch.quals, nothing),
                                   batch.offsets.data_ptr(), n, table.data_ptr(), _lib.stream_handle(dev, stream)))
    _lib.for_stream(nothing, stream)


def qc_insert_device(indexer, batch, mate, hist, stream=None) -> None:
    """The insert lengths of the pairs of ``batch`` and ``mate``, record by record, ADDED into ``hist``, an
    int64[INSERT_WORDS] device tensor that the caller zeroed once: asynchronously, in one call.  Only the bases and
    their offsets are read."""
    import torch
    n = int(batch.n_records)
    for b in (batch, mate):
        _need_batch("qc_insert_device", b, n)
    _need_table("qc_insert_device", hist, INSERT_WORDS)
    dev = batch.bases.device
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    check(lib().gf_qc_insert_device(indexer._handle(), _address(batch.bases, nothing), batch.offsets.data_ptr(),
                                    _address(mate.bases, nothing), mate.offsets.data_ptr(), n, hist.data_ptr(),
                                    _lib.stream_handle(dev, stream)))
    _lib.for_stream(nothing, stream)


def _rate(part: int, whole: int) -> float:
    return part / whole if whole else 0.0


class QcResult(NamedTuple):
    """What a ``ReadQc`` measured, on the host.  ``before`` / ``after``: per side (R1, then R2 of pairs) the int64
    array of ``gf_qc_stats_device``; ``insert``: the int64 array of ``gf_qc_insert_device``, None when it was not
    taken (single-end reads, ``insert_size=False``).  The derived figures are methods."""
    before: Tuple[np.ndarray, ...]
    after: Tuple[np.ndarray, ...]
    insert: Optional[np.ndarray] = None

    def tables(self, stage: str) -> Tuple[np.ndarray, ...]:
        if stage not in STAGES:
            raise ValueError("stage must be 'before' or 'after', not %r" % (stage,))
        return self.before if stage == "before" else self.after

    @staticmethod
    def length_hist(table) -> np.ndarray:
        return np.asarray(table[:CYCLES + 1])

    @staticmethod
    def cycles(table) -> np.ndarray:
        """cycle[513][8] of a side's table."""
        return np.asarray(table[CYCLES + 1:]).reshape(CYCLES + 1, COLUMNS)

    def summary(self, stage: str) -> dict:
        """``total_reads``, ``total_bases``, ``q20_bases``, ``q30_bases``, ``q20_rate``, ``q30_rate``,
        ``read1_mean_length`` (with pairs ``read2_mean_length``) and ``gc_content`` of a stage, both sides together.  A
        record of length 0 is not a read; a rate over 0 bases is 0.0; a mean length is rounded down."""
        tables = self.tables(stage)
        reads = [int(self.length_hist(t)[1:].sum()) for t in tables]
        cyc = [self.cycles(t) for t in tables]
        bases = [int(c[:, COL_A:COL_N + 1].sum()) for c in cyc]
        q20, q30 = (sum(int(c[:, col].sum()) for c in cyc) for col in (COL_Q20, COL_Q30))
        gc = sum(int(c[:, COL_G].sum() + c[:, COL_C].sum()) for c in cyc)
        out = {"total_reads": sum(reads), "total_bases": sum(bases), "q20_bases": q20, "q30_bases": q30,
               "q20_rate": _rate(q20, sum(bases)), "q30_rate": _rate(q30, sum(bases))}
        for k, (r, b) in enumerate(zip(reads, bases)):
            out["read%d_mean_length" % (k + 1)] = b // r if r else 0
        out["gc_content"] = _rate(gc, sum(bases))
        return out

    def curves(self, stage: str, side: int) -> dict:
        """``total_cycles`` — the longest read seen, at most 512 — and over the cycles below it ``quality_curves.mean``
        and ``content_curves`` for A, T, C, G, N and GC, each a share of the bases at that cycle."""
        table = self.tables(stage)[side]
        seen = np.nonzero(self.length_hist(table)[1:])[0]
        total = int(seen[-1]) + 1 if len(seen) else 0
        rows = self.cycles(table)[:min(total, CYCLES)]
        at = [int(r[COL_A:COL_N + 1].sum()) for r in rows]
        share = lambda cols: [_rate(sum(int(r[c]) for c in cols), n) for r, n in zip(rows, at)]   # noqa: E731
        return {"total_cycles": total,
                "quality_curves": {"mean": share([COL_QUAL_SUM])},
                "content_curves": {"A": share([COL_A]), "T": share([COL_T]), "C": share([COL_C]), "G": share([COL_G]),
                                   "N": share([COL_N]), "GC": share([COL_G, COL_C])}}

    def insert_size(self) -> Optional[dict]:
        """``peak``: the smallest I >= 30 with the largest count, 0 when no pair has an insert; ``unknown``: the pairs
        without an insert and the unmeasured ones; ``histogram``: entry I the pairs with the insert I, up to the
        largest one seen (entry 0: the pairs without).  None when the histogram was not taken."""
        if self.insert is None:
            return None
        h = [int(x) for x in self.insert]
        measured = h[:INSERT_UNMEASURED]
        top = max(measured[INSERT_MIN:], default=0)
        last = max((i for i in range(INSERT_MIN, INSERT_UNMEASURED) if measured[i]), default=0)
        return {"peak": measured.index(top, INSERT_MIN) if top else 0, "unknown": h[0] + h[INSERT_UNMEASURED],
                "histogram": measured[:last + 1]}


class ReadQc:
    """The collector a scan adds into.  It owns the device tables — before and after, per side, and the insert
    histogram — allocated and zeroed at first use on the index's device; ``ValueError`` for a second device.
    ``insert_size``: whether the pairs' insert histogram is taken (at "before": on the reads as the sequencer wrote
    them)."""

    def __init__(self, insert_size: bool = True):
        if not isinstance(insert_size, bool):
            raise ValueError("ReadQc.insert_size must be True or False, not %r" % (insert_size,))
        self.insert_size = insert_size
        self._block = None       # int64[4 SIDE_WORDS + INSERT_WORDS]: before R1, R2, after R1, R2, the histogram
        self._sides = 0
        self._stages = set()
        self._inserts = False

    def _table(self, stage: str, side: int):
        at = (STAGES.index(stage) * 2 + side) * SIDE_WORDS
        return self._block[at:at + SIDE_WORDS]

    def _hist(self):
        return self._block[4 * SIDE_WORDS:]

    def measure(self, indexer, stage: str, *batches, stream=None) -> None:
        """One ``FastqBatch`` (single-end) or two (R1, R2) added to the tables of ``stage``, "before" or "after";
        with two at "before" and ``insert_size`` their insert lengths too.  Asynchronous."""
        import torch
        if stage not in STAGES:
            raise ValueError("stage must be 'before' or 'after', not %r" % (stage,))
        if len(batches) not in (1, 2):
            raise ValueError("measure takes one batch or a pair of them, not %d" % len(batches))
        dev = torch.device("cuda", indexer.info()["device"])
        if self._block is None:
            self._block = torch.zeros(4 * SIDE_WORDS + INSERT_WORDS, dtype=torch.int64, device=dev)
        elif self._block.device != dev:
            raise ValueError("this ReadQc holds its tables on %s; a scan on %s needs one of its own"
                             % (self._block.device, dev))
        for side, b in enumerate(batches):
            qc_stats_device(indexer, b, self._table(stage, side), stream)
        if stage == "before" and len(batches) == 2 and self.insert_size:
            qc_insert_device(indexer, batches[0], batches[1], self._hist(), stream)
            self._inserts = True
        self._sides = max(self._sides, len(batches))
        self._stages.add(stage)

    def result(self) -> QcResult:
        """Synchronises the device and reads the tables back, once.  A scan that ran neither trimming nor filter did
        not measure "after": it gets the numbers of "before"."""
        sides = max(self._sides, 1)
        if self._block is None:
            block = np.zeros(4 * SIDE_WORDS + INSERT_WORDS, dtype=np.int64)
        else:
            import torch
            torch.cuda.synchronize(self._block.device)
            block = self._block.cpu().numpy()
        side = lambda k: block[k * SIDE_WORDS:(k + 1) * SIDE_WORDS].copy()   # noqa: E731
        before = tuple(side(k) for k in range(sides))
        after = tuple(side(2 + k) for k in range(sides)) if "after" in self._stages else tuple(t.copy() for t in before)
        return QcResult(before, after, block[4 * SIDE_WORDS:].copy() if self._inserts else None)


def need_read_qc(x) -> Optional[ReadQc]:
    """``x`` when it is None or a ``ReadQc``; ``ValueError`` for anything else."""
    if x is None or isinstance(x, ReadQc):
        return x
    raise ValueError("qc must be None or a ReadQc, not %r" % (x,))


# fastp's name for what a counter of a scan counts (read_filter.COUNTER_KEYS, adapter_trim.ADAPTER_COUNTER_KEYS);
# mate_failed_reads, cut_by_overlap, cut_by_sequence and overlapping_pairs are this project's own
FILTERING_RESULT = (("passed_filter_reads", "reads_passed"), ("low_quality_reads", "reads_low_quality"),
                    ("too_many_N_reads", "reads_too_many_n"), ("too_short_reads", "reads_too_short"),
                    ("mate_failed_reads", "reads_mate_failed"))
ADAPTER_CUTTING = (("adapter_trimmed_reads", "adapter_reads_cut"), ("adapter_trimmed_bases", "adapter_bases_cut"),
                   ("cut_by_overlap", "adapter_cut_by_overlap"), ("cut_by_sequence", "adapter_cut_by_sequence"),
                   ("overlapping_pairs", "adapter_overlapping_pairs"))


OVERLAP_CORRECTION = (("overlapping_pairs", "correction_overlapping_pairs"),
                      ("pairs_with_differences", "correction_pairs_with_diffs"), ("corrected_reads", "corrected_reads"),
                      ("corrected_bases", "corrected_bases"), ("differences_left", "correction_diffs_left"))


UMI_COUNTS = (("tagged_reads", "umi_reads_tagged"), ("reads_without_umi", "umi_missing"), ("umis_with_N", "umi_with_n"),
              ("cut_bases", "umi_bases_cut"), ("too_short_reads", "umi_too_short"))


def report_document(result: QcResult, counters: Optional[dict] = None, duplication=None, umi=None) -> dict:
    """The QC document as a dict, in the order ``report_json`` writes it.  ``duplication``: the ``DedupResult`` of the
    scan's ``Dedup``.  ``umi``: the scan's ``Umi``."""
    doc = {"summary": {"before_filtering": result.summary("before"), "after_filtering": result.summary("after")}}
    if counters is not None and "reads_passed" in counters:
        doc["filtering_result"] = {name: int(counters[key]) for name, key in FILTERING_RESULT}
    if counters is not None and "adapter_reads_cut" in counters:
        doc["adapter_cutting"] = {name: int(counters[key]) for name, key in ADAPTER_CUTTING}
    if counters is not None and "corrected_reads" in counters:
        doc["overlap_correction"] = {name: int(counters[key]) for name, key in OVERLAP_CORRECTION}
    if counters is not None and "umi_reads_tagged" in counters:
        doc["umi"] = {**({} if umi is None else umi.describe()),
                      **{name: int(counters[key]) for name, key in UMI_COUNTS}}
    if duplication is not None:
        doc["duplication"] = {"rate": _rate(int(duplication.duplicates), int(duplication.checked)),
                              "histogram": [int(x) for x in duplication.histogram[1:]]}
    inserts = result.insert_size()
    if inserts is not None:
        doc["insert_size"] = inserts
    for stage in STAGES:
        for side in range(len(result.tables(stage))):
            doc["read%d_%s_filtering" % (side + 1, stage)] = result.curves(stage, side)
    return doc


def report_json(result: QcResult, counters: Optional[dict] = None, duplication=None, umi=None) -> str:
    """This project's own QC document, with fastp's key names where the statistic is the same: ``summary`` with
    ``before_filtering`` / ``after_filtering`` (``QcResult.summary``); with ``counters`` of a scan that ran them
    ``filtering_result`` (the read filter's counts), ``adapter_cutting`` (the trimming's), ``overlap_correction`` (the
    overlap correction's five counts, behind ``adapter_cutting``) and ``umi`` (the UMI step's five
    counts, and with ``umi``, the scan's ``umi.Umi``, its ``source``, ``length`` and ``skip`` in front); with ``duplication``, a
    ``dedup.DedupResult``, ``duplication``: the ``rate``, duplicates over the records checked (0.0 over 0), and the
    ``histogram``, entry c - 1 the keys offered c times, the last one those offered 31 times or more; ``insert_size``
    (``QcResult.insert_size``) when it was taken; and ``read1_before_filtering``, ``read2_before_filtering``,
    ``read1_after_filtering``, ``read2_after_filtering`` (``QcResult.curves``; read2 with pairs).  Compatibility with
    an outside parser is not claimed."""
    return json.dumps(report_document(result, counters, duplication, umi), indent=1) + "\n"
