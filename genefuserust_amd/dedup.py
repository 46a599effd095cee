"""Duplicate reads removed on the device, and the duplication rate, opt-in: the ``gf_dd_*`` calls of libgfdedup.so
(include/gf_dedup.h, which states the predicate).

Deep cell-free-DNA panels hold many PCR duplicates; the reference collapses them only at the very end, per fusion and by
position (``FusionResult.calc_unique``).  Here the records are keyed while they sit in HBM behind the read filter — a
64-bit hash of the folded bases of a read, or of both mates of a pair — and looked up in an open-addressed hash table in
HBM that lives across calls.  Of the records with one key the one with the lowest index in file order stays; every other
one becomes a record of length 0, with its mate.  The record count, order and indices stay, so the names and the original
records of a scan's matches are gathered from the FASTQ text as before.  Two distinct records share a key with
probability about n^2 / 2^65.  A feature outside the reference, off unless a ``Dedup`` is handed to a route.
libgfdedup.so is a library of its own on top of libgfmatch.so's public C ABI (genefuserust_amd/scan_csrc/).  No CPU
fallback: without the libraries and a GPU every device call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Tuple

from . import _lib

DD_LIB_PATH = os.path.join(_lib._HERE, "libgfdedup.so")

LEVELS, TOTALS, MIN_SLOTS = 32, 6, 1024
NO_INDEX = (1 << 63) - 1
# the keys the totals of a deduplicated scan go by, in the scan's own units (pairs or reads)
DEDUP_COUNTER_KEYS = ("dedup_checked", "dedup_unique", "dedup_duplicates", "dedup_bases_removed")

_vp, _i64 = C.c_void_p, C.c_int64
# libgfdedup.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfdedup.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(DD_LIB_PATH, "duplicate removal", "gf_dd_last_error", {
    "gf_dd_keys_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "gf_dd_insert_device": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "gf_dd_workspace_bytes": (_i64, [_i64]),
    "gf_dd_remove_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "gf_dd_rehash_device": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    "gf_dd_histogram_device": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "gf_dd_last_error": (C.c_char_p, []),
})


class Table(NamedTuple):
    """The three device arrays of a table: ``keys`` int64[slots] (the uint64 keys' bits, 0 = empty), ``first``
    int64[slots] (``NO_INDEX`` = empty), ``count`` int32[slots] (the uint32 counts' bits) or None."""
    keys: object
    first: object
    count: object

    @property
    def slots(self) -> int:
        return int(self.keys.numel())


def empty_table(slots: int, dev, counted: bool = True) -> Table:
    import torch
    return Table(torch.zeros(slots, dtype=torch.int64, device=dev),
                 torch.full((slots,), NO_INDEX, dtype=torch.int64, device=dev),
                 torch.zeros(slots, dtype=torch.int32, device=dev) if counted else None)


def _need_batch(what: str, b, n: int, quals: bool) -> None:
    import torch
    _lib.need_device_tensors(what, b.bases, b.offsets, *([b.quals] if quals else []))
    assert b.bases.dtype == torch.uint8 and b.offsets.dtype == torch.int64
    assert b.bases.is_contiguous() and b.offsets.is_contiguous()
    assert int(b.n_records) == n and b.offsets.numel() >= n + 1


def _need_table(what: str, table: Table) -> None:
    import torch
    _lib.need_device_tensors(what, table.keys, table.first, *([] if table.count is None else [table.count]))
    assert table.keys.dtype == torch.int64 and table.first.dtype == torch.int64 and table.first.numel() == table.slots
    assert table.count is None or (table.count.dtype == torch.int32 and table.count.numel() == table.slots)


def _address(t, nothing):
    # (records without a base: an empty tensor has no address, and the library wants one with records)
    return (t if t.numel() else nothing).data_ptr()


def _ptr(t):
    return None if t is None else t.data_ptr()


def keys_device(indexer, batch, mate=None, stream=None):
    """K of every record of ``batch`` (a ``FastqBatch``; only bases and offsets are read) — with ``mate`` of the pairs
    of both: an int64[n] device tensor holding the uint64 keys' bits, 0 for a record with no bases.  Asynchronous."""
    import torch
    n = int(batch.n_records)
    sides = [batch] + ([mate] if mate is not None else [])
    for b in sides:
        _need_batch("keys_device", b, n, False)
    dev = batch.bases.device
    rec_keys = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    ptrs = [[_address(b.bases, nothing), b.offsets.data_ptr()] for b in sides] + ([[None] * 2] if mate is None else [])
    check(lib().gf_dd_keys_device(indexer._handle(), *ptrs[0], *ptrs[1], n, rec_keys.data_ptr(),
                                  _lib.stream_handle(dev, stream)))
    for t in (rec_keys, nothing):
        _lib.for_stream(t, stream)
    return rec_keys[:n]


def insert_device(indexer, rec_keys, first_index: int, table: Table, totals, stream=None):
    """The keys found or placed in ``table``, record i at the global index ``first_index + i``; ``totals``
    (int64[6], device) is added into.  Returns the int64[n] device tensor of every record's slot, -1 for key 0."""
    import torch
    _lib.need_device_tensors("insert_device", rec_keys, totals)
    _need_table("insert_device", table)
    assert rec_keys.dtype == torch.int64 and rec_keys.is_contiguous()
    assert totals.dtype == torch.int64 and totals.numel() == TOTALS
    n, dev = int(rec_keys.numel()), table.keys.device
    rec_slot = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev)
    check(lib().gf_dd_insert_device(indexer._handle(), rec_keys.data_ptr() if n else None, n, int(first_index),
                                    table.keys.data_ptr(), table.first.data_ptr(), _ptr(table.count), table.slots,
                                    rec_slot.data_ptr(), totals.data_ptr(), _lib.stream_handle(dev, stream)))
    return _lib.for_stream(rec_slot, stream)[:n]


def remove_device(indexer, rec_slot, first_index: int, table: Table, totals, batch, mate=None, stream=None):
    """The duplicates among the records of ``batch`` (the full FASTQ cut) — with ``mate`` the pairs of both — emptied,
    behind the ``insert_device`` call that gave ``rec_slot``: (batch, [mate,] dup).  The batches have ``bases``,
    ``quals`` and ``offsets`` replaced by the survivors and ``qual_off`` None; ``dup``: the uint8[n] device tensor, 1 for
    a duplicate.  ``totals`` is added into."""
    import torch
    sides = [batch] + ([mate] if mate is not None else [])
    n = int(batch.n_records)
    for b in sides:
        if b.qual_off is not None:
            raise ValueError("remove_device takes the full FASTQ cut: the qualities at the bases' offsets")
        _need_batch("remove_device", b, n, True)
        assert b.quals.dtype == torch.uint8 and b.quals.is_contiguous() and b.quals.numel() >= b.bases.numel()
    _lib.need_device_tensors("remove_device", rec_slot, totals)
    _need_table("remove_device", table)
    assert rec_slot.dtype == torch.int64 and rec_slot.numel() == n and totals.numel() == TOTALS
    L = lib()
    dev = batch.bases.device
    ws_bytes = int(L.gf_dd_workspace_bytes(n))
    ws = _lib.workspace(ws_bytes, dev, stream)
    dup = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    out = [(torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.zeros(n + 1, dtype=torch.int64, device=dev)) for b in sides]
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    ptrs = [[_address(t, nothing) for t in (b.bases, b.quals)] + [b.offsets.data_ptr()]
            for b in sides] + ([[None] * 3] if mate is None else [])
    outs = [[t.data_ptr() for t in o] for o in out] + ([[None] * 3] if mate is None else [])
    check(L.gf_dd_remove_device(indexer._handle(), *ptrs[0], *ptrs[1], n, int(first_index),
                                rec_slot.data_ptr() if n else None, table.first.data_ptr(), ws.data_ptr(), ws_bytes,
                                *outs[0], *outs[1], dup.data_ptr(), totals.data_ptr(), _lib.stream_handle(dev, stream)))
    for t in [x for o in out for x in o] + [dup, nothing]:
        _lib.for_stream(t, stream)
    new = [b._replace(bases=ob[:b.bases.numel()], quals=oq[:b.bases.numel()], offsets=off, qual_off=None)
           for b, (ob, oq, off) in zip(sides, out)]
    return (*new, dup[:n])


def rehash_device(indexer, old: Table, new: Table, stream=None) -> None:
    """Every entry of ``old`` placed in ``new``, a larger table, which the call empties first.  Asynchronous."""
    _need_table("rehash_device", old)
    _need_table("rehash_device", new)
    check(lib().gf_dd_rehash_device(indexer._handle(), old.keys.data_ptr(), old.first.data_ptr(), _ptr(old.count),
                                    old.slots, new.keys.data_ptr(), new.first.data_ptr(), _ptr(new.count), new.slots,
                                    _lib.stream_handle(old.keys.device, stream)))


def histogram_device(indexer, table: Table, hist, stream=None) -> None:
    """The keys of ``table`` by how often they were offered, ADDED into ``hist`` (int64[32], device)."""
    import torch
    _need_table("histogram_device", table)
    _lib.need_device_tensors("histogram_device", hist)
    assert hist.dtype == torch.int64 and hist.numel() == LEVELS and hist.is_contiguous()
    check(lib().gf_dd_histogram_device(indexer._handle(), table.keys.data_ptr(), _ptr(table.count), table.slots,
                                       hist.data_ptr(), _lib.stream_handle(table.keys.device, stream)))


class DedupResult(NamedTuple):
    """What a ``Dedup`` has seen: ``checked`` records with bases, ``unique`` keys among them, ``duplicates`` — the
    rest —, the ``bases_removed`` with them (0 with ``remove=False``), and ``histogram``: entry c the keys offered c
    times, entry 31 those offered 31 times or more, entry 0 always 0."""
    checked: int
    unique: int
    duplicates: int
    bases_removed: int
    histogram: Tuple[int, ...]

    def rate(self) -> float:
        return self.duplicates / self.checked if self.checked else 0.0


def _power_of_two(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, int) and x > 0 and x & (x - 1) == 0


class Dedup:
    """The collector a scan deduplicates through; the caller owns it, as a ``ReadQc``.  It owns the table — allocated at
    first use on the index's device, ``ValueError`` for a second device — and counts what it has been offered: that
    count is the global index of the next call's first record.  So one ``Dedup`` handed to the scans of two lanes removes
    the duplicates across them, and one handed the same file twice removes every record of the second pass.

    ``remove``: False only counts — the records go on as they came, and no gather is queued.  ``slots``: the table's
    first size, a power of two of at least 1024; before an insert that could take the table past half full it is
    replaced by the next sufficient power of two and rehashed, up to ``max_slots`` (``RuntimeError`` past it).  The table
    takes 20 bytes a slot."""

    def __init__(self, remove: bool = True, slots: int = 1 << 22, max_slots: int = 1 << 31):
        if not isinstance(remove, bool):
            raise ValueError("Dedup.remove must be True or False, not %r" % (remove,))
        for name, v in (("slots", slots), ("max_slots", max_slots)):
            if not _power_of_two(v) or v < MIN_SLOTS:
                raise ValueError("Dedup.%s must be a power of two of at least %d, not %r" % (name, MIN_SLOTS, v))
        if max_slots < slots:
            raise ValueError("Dedup.max_slots (%d) is below slots (%d)" % (max_slots, slots))
        self.remove, self.slots, self.max_slots = remove, slots, max_slots
        self.offered = 0          # records offered so far: the next call's first_index
        self._table: Optional[Table] = None
        self._totals = None       # int64[6], summed over the calls
        self._hist = None         # int64[32], the table's histogram behind the last call

    def slots_for(self, n: int) -> int:
        """The size the table needs before ``n`` more records are offered: the smallest power of two, not below the
        present size, that they leave at most half full.  ``RuntimeError`` past ``max_slots``."""
        slots = self.slots
        while self.offered + n > slots // 2:
            slots *= 2
        if slots > self.max_slots:
            raise RuntimeError("Dedup: %d records offered and %d more need a table of %d slots; max_slots is %d"
                               % (self.offered, n, slots, self.max_slots))
        return slots

    def _prepare(self, indexer, n: int, stream) -> None:
        import torch
        dev = torch.device("cuda", indexer.info()["device"])
        if self._table is not None and self._table.keys.device != dev:
            raise ValueError("this Dedup holds its table on %s; a scan on %s needs one of its own"
                             % (self._table.keys.device, dev))
        slots = self.slots_for(n)
        if self._table is None:
            self._table = empty_table(slots, dev)
            self._totals = torch.zeros(TOTALS, dtype=torch.int64, device=dev)
        elif slots != self.slots:
            old, self._table = self._table, empty_table(slots, dev)
            rehash_device(indexer, old, self._table, stream)
            for t in old:   # (freed in stream order: behind the rehash)
                _lib.for_stream(t, stream)
        self.slots = slots

    def apply(self, indexer, *batches, stream=None, umi_codes=None):
        """One ``FastqBatch`` (single-end) or two (R1, R2) keyed, looked up and, with ``remove``, emptied of duplicates:
        (batches, totals) — the batches as ``read_filter.filter_reads_device`` leaves them (with ``remove=False`` as
        they came), ``totals`` the int64[6] device tensor of this call alone.  ``umi_codes``: the int64[n] device tensor
        of the records' UMI codes (umi.py), mixed into the keys between the hashing and the table (``umi.mix_keys_device``)
        — two records are then duplicates when their bases and their UMIs are equal; None (the default): the calls
        queued are the same as ever.  Asynchronous."""
        import torch
        if len(batches) not in (1, 2):
            raise ValueError("apply takes one batch or a pair of them, not %d" % len(batches))
        if self.remove and any(b.qual_off is not None for b in batches):   # (before the table is touched)
            raise ValueError("Dedup.apply takes the full FASTQ cut: the qualities at the bases' offsets")
        n = int(batches[0].n_records)
        self._prepare(indexer, n, stream)
        totals = torch.zeros(TOTALS, dtype=torch.int64, device=self._table.keys.device)
        rec_keys = keys_device(indexer, *batches, stream=stream)
        if umi_codes is not None:
            from .umi import mix_keys_device
            if int(umi_codes.numel()) != n:
                raise ValueError("apply: %d UMI codes for %d records" % (umi_codes.numel(), n))
            mix_keys_device(indexer, rec_keys, umi_codes, stream)
        rec_slot = insert_device(indexer, rec_keys, self.offered, self._table, totals, stream)
        if self.remove:
            *batches, _ = remove_device(indexer, rec_slot, self.offered, self._table, totals, *batches, stream=stream)
        self.offered += n
        # the histogram of the table as it now stands, for ``result``, which has no index to call with: one pass over
        # the table's keys and counts a call
        self._hist = _lib.for_stream(torch.zeros(LEVELS, dtype=torch.int64, device=totals.device), stream)
        histogram_device(indexer, self._table, self._hist, stream)
        if stream is None:
            self._totals += totals
        else:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=totals.device)):
                self._totals += totals
        return tuple(batches), _lib.for_stream(totals, stream)

    def result(self) -> DedupResult:
        """Synchronises the device and reads the totals and the histogram back, once.  ``RuntimeError`` when a probe
        failed: the table was full, which growing at half full rules out."""
        if self._table is None:
            return DedupResult(0, 0, 0, 0, (0,) * LEVELS)
        import torch
        dev = self._table.keys.device
        torch.cuda.synchronize(dev)
        both = torch.cat([self._totals, self._hist]).cpu().tolist()   # (the one read-back)
        totals, hist = both[:TOTALS], both[TOTALS:]
        if totals[5]:
            raise RuntimeError("Dedup: %d probes found no slot in a table of %d" % (totals[5], self.slots))
        c = dedup_totals_counters(totals, self.remove)
        return DedupResult(c["dedup_checked"], c["dedup_unique"], c["dedup_duplicates"], c["dedup_bases_removed"],
                           tuple(int(x) for x in hist))


def need_dedup(x) -> Optional[Dedup]:
    """``x`` when it is None or a ``Dedup``; ``ValueError`` for anything else."""
    if x is None or isinstance(x, Dedup):
        return x
    raise ValueError("dedup must be None or a Dedup, not %r" % (x,))


def dedup_totals_counters(totals, remove: bool = True) -> dict:
    """The four counters of a call's or a scan's totals (a sequence of six integers), under the keys a deduplicated
    scan reports.  ``remove=False``: nothing was removed and so nothing counted as removed; the duplicates are the
    hashed records less the new keys."""
    t = [int(x) for x in totals]
    return dict(zip(DEDUP_COUNTER_KEYS, (t[1], t[2], t[3] if remove else t[1] - t[2], t[4] if remove else 0)))
