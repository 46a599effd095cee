"""Unique molecular identifiers cut on the device and keyed into the duplicate removal, opt-in: the ``gf_um_*`` calls
of libgfumi.so (include/gf_umi.h, which states the predicate).

Deep cell-free-DNA panels carry UMIs: a few random bases ligated to a molecule before the PCR.  cfDNA is cut at preferred
positions, so two molecules with the same bases are common at panel depth, and only the UMI tells a PCR copy from a
second molecule.  Inline UMIs — the first bases of R1, R2 or both, often with a spacer behind them — are taken off the
records while they sit in HBM, so that they are neither merged, nor seeded, nor mapped as if they were genome; a UMI the
sequencer's software wrote behind the last ':' of the read's name is read from the FASTQ text.  Either way every record
gets a 64-bit code, and ``Dedup.apply(..., umi_codes=codes)`` mixes it into the record's key: PCR copies of one molecule
are still duplicates, two molecules with the same bases no longer are.  The record count, order and indices stay.  A
feature outside the reference, off unless a ``Umi`` is handed to a route.  libgfumi.so is a library of its own on top of
libgfmatch.so's public C ABI (genefuserust_amd/scan_csrc/).  No CPU fallback: without the libraries and a GPU every
device call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import _lib

UM_LIB_PATH = os.path.join(_lib._HERE, "libgfumi.so")

NAME, READ1, READ2, PER_READ = 0, 1, 2, 3
SOURCES = {"name": NAME, "read1": READ1, "read2": READ2, "per_read": PER_READ}
MAX_LEN, MAX_SKIP, MAX_FIELD, TOTALS = 32, 32, 64, 7
# the keys the totals of a scan with UMIs go by, in the scan's own units (pairs or reads): totals [1], [2], [3], [4], [5]
UMI_COUNTER_KEYS = ("umi_reads_tagged", "umi_missing", "umi_with_n", "umi_bases_cut", "umi_too_short")


class GfUmSettings(C.Structure):
    _fields_ = [("source", C.c_int32), ("length", C.c_int32), ("skip", C.c_int32)]


_vp, _i64 = C.c_void_p, C.c_int64
# libgfumi.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfumi.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(UM_LIB_PATH, "UMI handling", "gf_um_last_error", {
    "gf_um_workspace_bytes": (_i64, [_i64]),
    "gf_um_cut_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _vp]),
    "gf_um_names_device": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp]),
    "gf_um_mix_keys_device": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "gf_um_last_error": (C.c_char_p, []),
})


def _is_int(x) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


class Umi:
    """Where a library's UMIs are.  ``source``: "name" — behind the last ':' of the first token of the read's name
    (for pairs R1's), ``length`` and ``skip`` 0; "read1", "read2", "per_read" — the first ``length`` (1 .. 32) bases of
    R1, of R2, or of both, with ``skip`` (0 .. 32) bases of spacer behind them that are cut off too.  Single-end input
    takes "per_read" as "read1" and refuses "read2".  ``ValueError`` for anything else."""

    def __init__(self, source: str = "name", length: int = 0, skip: int = 0):
        if not isinstance(source, str) or source not in SOURCES:
            raise ValueError("Umi.source must be one of %s, not %r" % (", ".join(map(repr, SOURCES)), source))
        if not _is_int(length) or not _is_int(skip):
            raise ValueError("Umi.length and Umi.skip must be integers, not %r and %r" % (length, skip))
        if source == "name":
            if length != 0 or skip != 0:
                raise ValueError("Umi(source='name') takes no length and no skip: the name holds the whole UMI")
        else:
            if not 1 <= length <= MAX_LEN:
                raise ValueError("Umi.length must be 1 .. %d for source %r, not %r" % (MAX_LEN, source, length))
            if not 0 <= skip <= MAX_SKIP:
                raise ValueError("Umi.skip must be 0 .. %d, not %r" % (MAX_SKIP, skip))
        self.source, self.length, self.skip = source, length, skip

    @property
    def inline(self) -> bool:
        return self.source != "name"

    def need_sides(self, sides: int) -> "Umi":
        """``ValueError`` for "read2" with single-end input."""
        if self.source == "read2" and sides == 1:
            raise ValueError("umi: source 'read2' needs paired-end input; single-end reads have no R2")
        return self

    def settings(self) -> GfUmSettings:
        return GfUmSettings(SOURCES[self.source], self.length, self.skip)

    def describe(self) -> dict:
        return {"source": self.source, "length": self.length, "skip": self.skip}

    def __repr__(self) -> str:
        return "Umi(source=%r, length=%d, skip=%d)" % (self.source, self.length, self.skip)


def need_umi(x) -> Optional[Umi]:
    """``x`` when it is None or a ``Umi``; ``ValueError`` for anything else."""
    if x is None or isinstance(x, Umi):
        return x
    raise ValueError("umi must be None or a Umi, not %r" % (x,))


def umi_totals_counters(totals) -> dict:
    """The five counters of a call's or a scan's totals (a sequence of seven integers), under the keys a scan with UMIs
    reports."""
    t = [int(x) for x in totals]
    return dict(zip(UMI_COUNTER_KEYS, (t[1], t[2], t[3], t[4], t[5])))


def _address(t, nothing):
    # (records without a base: an empty tensor has no address, and the library wants one with records)
    return (t if t.numel() else nothing).data_ptr()


def cut_umis_device(indexer, config: Umi, batch, mate=None, stream=None):
    """The inline UMIs of the records of ``batch`` (the full FASTQ cut) — with ``mate`` the pairs of both — taken off:
    (batch, [mate,] codes, totals).  The batches have ``bases``, ``quals`` and ``offsets`` replaced by the cut records
    and ``qual_off`` None; ``codes``: the int64[n] device tensor of the uint64 codes' bits, 0 for a record emptied as too
    short; ``totals``: the int64[7] device tensor of this call.  Asynchronous."""
    import torch
    if not isinstance(config, Umi) or not config.inline:
        raise ValueError("cut_umis_device takes a Umi with an inline source, not %r" % (config,))
    sides = [batch] + ([mate] if mate is not None else [])
    config.need_sides(len(sides))
    n = int(batch.n_records)
    for b in sides:
        if b.qual_off is not None:
            raise ValueError("cut_umis_device takes the full FASTQ cut: the qualities at the bases' offsets")
        _lib.need_device_tensors("cut_umis_device", b.bases, b.quals, b.offsets)
        assert b.bases.dtype == torch.uint8 and b.quals.dtype == torch.uint8 and b.offsets.dtype == torch.int64
        assert b.bases.is_contiguous() and b.quals.is_contiguous() and b.offsets.is_contiguous()
        assert int(b.n_records) == n and b.offsets.numel() >= n + 1 and b.quals.numel() >= b.bases.numel()
    L = lib()
    dev = batch.bases.device
    ws_bytes = int(L.gf_um_workspace_bytes(n))
    ws = _lib.workspace(ws_bytes, dev, stream)
    codes = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    totals = torch.zeros(TOTALS, dtype=torch.int64, device=dev)
    out = [(torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.zeros(n + 1, dtype=torch.int64, device=dev)) for b in sides]
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    ptrs = [[_address(t, nothing) for t in (b.bases, b.quals)] + [b.offsets.data_ptr()]
            for b in sides] + ([[None] * 3] if mate is None else [])
    outs = [[t.data_ptr() for t in o] for o in out] + ([[None] * 3] if mate is None else [])
    settings = config.settings()
    check(L.gf_um_cut_device(indexer._handle(), C.addressof(settings), *ptrs[0], *ptrs[1], n, ws.data_ptr(), ws_bytes,
                             *outs[0], *outs[1], codes.data_ptr(), totals.data_ptr(),
                             _lib.stream_handle(dev, stream)))
    for t in [x for o in out for x in o] + [codes, totals, nothing]:
        _lib.for_stream(t, stream)
    new = [b._replace(bases=ob[:b.bases.numel()], quals=oq[:b.bases.numel()], offsets=off, qual_off=None)
           for b, (ob, oq, off) in zip(sides, out)]
    return (*new, codes[:n], totals)


def name_umis_device(indexer, text, batch, stream=None):
    """The UMIs in the names of the records of ``batch``, cut (either way) from the FASTQ ``text`` on the device:
    (codes, totals) — ``codes`` the int64[n] device tensor of the uint64 codes' bits, 0 for a record whose name holds no
    UMI; ``totals`` the int64[7] device tensor of this call.  Moves no byte of the records.  Asynchronous."""
    import torch
    _lib.need_device_tensors("name_umis_device", text, batch.nl_pos)
    assert text.dtype == torch.uint8 and text.is_contiguous()
    assert batch.nl_pos.dtype == torch.int64 and batch.nl_pos.is_contiguous()
    n, newlines = int(batch.n_records), int(batch.n_newlines)
    assert batch.nl_pos.numel() >= newlines
    dev = text.device
    codes = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    totals = torch.zeros(TOTALS, dtype=torch.int64, device=dev)
    check(lib().gf_um_names_device(indexer._handle(), text.data_ptr() if text.numel() else None, int(text.numel()),
                                   batch.nl_pos.data_ptr() if newlines else None, newlines, n, codes.data_ptr(),
                                   totals.data_ptr(), _lib.stream_handle(dev, stream)))
    for t in (codes, totals):
        _lib.for_stream(t, stream)
    return codes[:n], totals


def mix_keys_device(indexer, rec_keys, codes, stream=None):
    """K' of every record, in place: ``rec_keys`` (int64[n], as ``dedup.keys_device`` gave them) mixed with ``codes``
    (int64[n]).  Returns ``rec_keys``.  Asynchronous."""
    import torch
    _lib.need_device_tensors("mix_keys_device", rec_keys, codes)
    assert rec_keys.dtype == torch.int64 and rec_keys.is_contiguous()
    assert codes.dtype == torch.int64 and codes.is_contiguous() and codes.numel() == rec_keys.numel()
    n = int(rec_keys.numel())
    check(lib().gf_um_mix_keys_device(indexer._handle(), rec_keys.data_ptr() if n else None,
                                      codes.data_ptr() if n else None, n,
                                      _lib.stream_handle(rec_keys.device, stream)))
    return rec_keys
