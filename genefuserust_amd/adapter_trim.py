"""Adapter trimming of reads on the device, by pair overlap and by sequence, opt-in: ``gf_at_trim_device`` of
libgfadapt.so (include/gf_adapter_trim.h).

A fragment shorter than the reads is read through into the adapter by both mates.  ``fast_merge`` only tries a tail of
R1 against the head of rc(R2) — an insert at least as long as the reads — so such a pair never merges, and each mate
carries an adapter tail into the mapping.  Here the records are cut to the insert while they sit in HBM between the
FASTQ cut and the read filter or the scan: a pair by the largest insert length at which the mates are each other's
reverse complement, a read without such a mate by the adapter's sequence.  The record count, order and indices stay,
so the names and the original records of a scan's matches are gathered from the FASTQ text as before.  A feature
outside the reference, off unless an ``AdapterTrim`` is handed to a route.  libgfadapt.so is a library of its own on
top of libgfmatch.so's public C ABI (genefuserust_amd/scan_csrc/).  No CPU fallback: without the libraries and a GPU
every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

from . import _lib

AT_LIB_PATH = os.path.join(_lib._HERE, "libgfadapt.so")

READ_MAX, ADAPTER_MAX, TOTALS = 512, 64, 6
UNTOUCHED, BY_OVERLAP, BY_SEQUENCE, OVERLAP_CLEAN = 0, 1, 2, 3
# what adapter_r1="illumina" / adapter_r2="illumina" stand for: the TruSeq adapters behind R1's and R2's insert
TRUSEQ_R1 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
TRUSEQ_R2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
# the keys the totals of a trimmed scan go by, behind "reads seen" (which ``pairs`` / ``reads`` already count)
ADAPTER_COUNTER_KEYS = ("adapter_reads_cut", "adapter_bases_cut", "adapter_cut_by_overlap", "adapter_cut_by_sequence",
                        "adapter_overlapping_pairs")


@dataclass(frozen=True)
class AdapterTrim:
    """The settings of the trimming (include/gf_adapter_trim.h says what each step does).  ``ValueError`` for what the
    library refuses: ``min_overlap`` outside 8 .. 512, a negative ``max_diff``, ``diff_percent`` outside 0 .. 100,
    ``min_adapter`` outside 4 .. 64, an adapter that is neither empty nor ``min_adapter`` .. 64 bases of ACGT, and
    ``overlap=False`` with no adapter.  "illumina" as an adapter stands for ``TRUSEQ_R1`` / ``TRUSEQ_R2``."""
    overlap: bool = True         # pairs are cut by the overlap of their mates
    adapter_r1: str = ""         # the adapter behind R1's (and a single-end read's) insert; "": none
    adapter_r2: str = ""         # the adapter behind R2's insert; "": none
    min_overlap: int = 30        # the fewest positions an accepted insert compares
    max_diff: int = 5            # the most differences of an accepted insert
    diff_percent: int = 20       # the share of differences of an accepted insert
    min_adapter: int = 10        # the fewest adapter bases looked for at a read's end

    def __post_init__(self):
        if not isinstance(self.overlap, bool):
            raise ValueError("AdapterTrim.overlap must be True or False, not %r" % (self.overlap,))
        limits = dict(min_overlap=(8, READ_MAX), max_diff=(0, 2 ** 31 - 1), diff_percent=(0, 100),
                      min_adapter=(4, ADAPTER_MAX))
        for name, (lo, hi) in limits.items():
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError("AdapterTrim.%s must be an integer in %d .. %d, not %r" % (name, lo, hi, v))
        for name, known in (("adapter_r1", TRUSEQ_R1), ("adapter_r2", TRUSEQ_R2)):
            v = getattr(self, name)
            if v == "illumina":
                v = known
                object.__setattr__(self, name, v)
            if not isinstance(v, str) or set(v) - set("ACGT") or (v and not self.min_adapter <= len(v) <= ADAPTER_MAX):
                raise ValueError("AdapterTrim.%s must be empty, \"illumina\" or %d .. %d bases of ACGT, not %r"
                                 % (name, self.min_adapter, ADAPTER_MAX, v))
        if not self.overlap and not self.adapter_r1 and not self.adapter_r2:
            raise ValueError("AdapterTrim: overlap=False with no adapter leaves nothing to do")


def need_adapter_trim(x) -> Optional[AdapterTrim]:
    """``x`` when it is None or an ``AdapterTrim``; ``ValueError`` for anything else."""
    if x is None or isinstance(x, AdapterTrim):
        return x
    raise ValueError("adapter_trim must be None or an AdapterTrim, not %r" % (x,))


class GfAtSettings(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ("overlap", "min_overlap", "max_diff", "diff_percent", "min_adapter",
                                               "adapter_r1_len", "adapter_r2_len")] + \
               [("adapter_r1", C.c_uint8 * ADAPTER_MAX), ("adapter_r2", C.c_uint8 * ADAPTER_MAX)]


def settings_of(config: AdapterTrim) -> GfAtSettings:
    """The library's struct for ``config``."""
    r1, r2 = config.adapter_r1.encode(), config.adapter_r2.encode()
    pad = lambda a: (C.c_uint8 * ADAPTER_MAX)(*a)   # noqa: E731
    return GfAtSettings(int(config.overlap), config.min_overlap, config.max_diff, config.diff_percent,
                        config.min_adapter, len(r1), len(r2), pad(r1), pad(r2))


_vp, _i64 = C.c_void_p, C.c_int64
# libgfadapt.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfadapt.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(AT_LIB_PATH, "adapter trimming", "gf_at_last_error", {
    "gf_at_workspace_bytes": (_i64, [_i64]),
    "gf_at_trim_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp]),
    "gf_at_last_error": (C.c_char_p, []),
})


def trim_adapters_device(indexer, config: AdapterTrim, batch, mate=None, stream=None, how: bool = False):
    """The trimming over the records of ``batch`` (a ``FastqBatch`` of the full cut: the qualities at the bases'
    offsets) — with ``mate`` the pairs of both, record by record — asynchronously, in one call.  Returns (batch, totals)
    or (batch, mate, totals): the batches with ``bases``, ``quals`` and ``offsets`` replaced by the kept prefixes and
    ``qual_off`` None, everything that locates the records in the FASTQ text as it was; ``totals``: the int64[6] device
    tensor of ``gf_at_trim_device``.  ``how``: the uint8 device tensor of every record's code follows (R1's, then
    R2's).  A single-end batch needs a config with ``adapter_r1``: ``ValueError`` without."""
    import torch
    need_adapter_trim(config)
    if config is None:
        raise ValueError("trim_adapters_device needs an AdapterTrim")
    if mate is None and not config.adapter_r1:
        raise ValueError("trim_adapters_device: single-end reads are trimmed by sequence, and adapter_trim has no "
                         "adapter_r1")
    sides = [batch] + ([mate] if mate is not None else [])
    n = int(batch.n_records)
    for b in sides:
        if b.qual_off is not None:
            raise ValueError("trim_adapters_device takes the full FASTQ cut: the qualities at the bases' offsets")
        _lib.need_device_tensors("trim_adapters_device", b.bases, b.quals, b.offsets)
        assert b.bases.dtype == torch.uint8 and b.quals.dtype == torch.uint8 and b.offsets.dtype == torch.int64
        assert b.bases.is_contiguous() and b.quals.is_contiguous() and b.offsets.is_contiguous()
        assert int(b.n_records) == n and b.offsets.numel() >= n + 1 and b.quals.numel() >= b.bases.numel()
    L = lib()
    dev = batch.bases.device
    ws_bytes = int(L.gf_at_workspace_bytes(n))
    ws = _lib.workspace(ws_bytes, dev, stream)
    totals = torch.zeros(TOTALS, dtype=torch.int64, device=dev)
    codes = torch.zeros(max(n * len(sides), 1), dtype=torch.uint8, device=dev)
    out = [(torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.zeros(n + 1, dtype=torch.int64, device=dev)) for b in sides]
    # (records without a base: an empty tensor has no address, and the library wants one with records)
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    ptrs = [[(t if t.numel() else nothing).data_ptr() for t in (b.bases, b.quals)] + [b.offsets.data_ptr()]
            for b in sides] + ([[None] * 3] if mate is None else [])
    outs = [[t.data_ptr() for t in o] for o in out] + ([[None] * 3] if mate is None else [])
    settings = settings_of(config)
    check(L.gf_at_trim_device(indexer._handle(), C.byref(settings), *ptrs[0], *ptrs[1], n, ws.data_ptr(), ws_bytes,
                              *outs[0], *outs[1], codes.data_ptr(), totals.data_ptr(), _lib.stream_handle(dev, stream)))
    for t in [x for o in out for x in o] + [totals, codes]:
        _lib.for_stream(t, stream)
    new = []
    for b, (ob, oq, off) in zip(sides, out):
        # (the kept bytes are known on the device only: the tensors keep the input's size, the offsets say what counts)
        new.append(b._replace(bases=ob[:b.bases.numel()], quals=oq[:b.bases.numel()], offsets=off, qual_off=None))
    return (*new, totals, codes[:n * len(sides)]) if how else (*new, totals)


def adapter_totals_counters(totals) -> dict:
    """The five counters of a trimming's totals (a sequence of six integers), under the keys a trimmed scan reports."""
    return dict(zip(ADAPTER_COUNTER_KEYS, (int(x) for x in list(totals)[1:])))
