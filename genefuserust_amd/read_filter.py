"""Quality filter and tail trimming of reads on the device, opt-in: ``gf_pp_filter_device`` of libgfprep.so
(include/gf_read_filter.h).

GeneFuse expects FASTQ that has been through a quality filter (fastp, AfterQC); the reference never looks at a quality
value outside ``fast_merge``.  Here that step runs on the records while they sit in HBM between the FASTQ cut and the
scan: poly-G tails and low-quality tails are cut off, and reads that are then too short, hold too many N or too many
low bases become records of length 0 — with their mates.  The record count, order and indices stay, so the names and
the original records of a scan's matches are gathered from the FASTQ text as before.  A feature outside the reference,
off unless a ``ReadFilter`` is handed to a route.  libgfprep.so is a library of its own on top of libgfmatch.so's public
C ABI (genefuserust_amd/scan_csrc/).  No CPU fallback: without the libraries and a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import astuple, dataclass, fields
from typing import Optional

from . import _lib

PP_LIB_PATH = os.path.join(_lib._HERE, "libgfprep.so")

WINDOW_MAX, PHRED_MAX = 64, 93
# the keys the totals of a filtered scan go by, behind "reads seen" (which ``pairs`` / ``reads`` already count)
COUNTER_KEYS = ("reads_passed", "reads_trimmed", "bases_trimmed", "reads_too_short", "reads_too_many_n",
                "reads_low_quality", "reads_mate_failed")


@dataclass(frozen=True)
class ReadFilter:
    """The settings of the filter (include/gf_read_filter.h says what each step does).  ``ValueError`` for what the
    library refuses: a negative value, a window above 64, a phred above 93, a percentage above 100, ``poly_g_min`` or
    ``length_required`` above ``GF_MAX_READ_LEN``."""
    poly_g_min: int = 10            # 0 switches poly-G trimming off
    cut_tail_window: int = 0        # 0: off; 1 .. 64 switches the tail cut on
    cut_tail_mean: int = 20         # the mean phred a tail window must reach
    length_required: int = 15       # the shortest read kept
    n_base_limit: int = 5           # the most N bases a kept read may have
    qualified_phred: int = 15       # a base below this is a low base
    unqualified_percent: int = 40   # the share of low bases allowed

    def __post_init__(self):
        limits = dict(poly_g_min=_lib.GF_MAX_READ_LEN, cut_tail_window=WINDOW_MAX, cut_tail_mean=PHRED_MAX,
                      length_required=_lib.GF_MAX_READ_LEN, n_base_limit=2 ** 31 - 1, qualified_phred=PHRED_MAX,
                      unqualified_percent=100)
        for f in fields(self):
            v = getattr(self, f.name)
            if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= limits[f.name]:
                raise ValueError("ReadFilter.%s must be an integer in 0 .. %d, not %r" % (f.name, limits[f.name], v))


def need_read_filter(x) -> Optional[ReadFilter]:
    """``x`` when it is None or a ``ReadFilter``; ``ValueError`` for anything else."""
    if x is None or isinstance(x, ReadFilter):
        return x
    raise ValueError("read_filter must be None or a ReadFilter, not %r" % (x,))


class GfPpSettings(C.Structure):
    _fields_ = [(f.name, C.c_int32) for f in fields(ReadFilter)]


_vp, _i64 = C.c_void_p, C.c_int64
# libgfprep.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfprep.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(PP_LIB_PATH, "read filter", "gf_pp_last_error", {
    "gf_pp_workspace_bytes": (_i64, [_i64]),
    "gf_pp_filter_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp]),
    "gf_pp_last_error": (C.c_char_p, []),
})


def filter_reads_device(indexer, config: ReadFilter, batch, mate=None, stream=None, reasons: bool = False):
    """The filter over the records of ``batch`` (a ``FastqBatch`` of the full cut: the qualities at the bases' offsets)
    — with ``mate`` the pairs of both, record by record — asynchronously, in one call.  Returns (batch, totals) or
    (batch, mate, totals): the batches with ``bases``, ``quals`` and ``offsets`` replaced by the kept prefixes (a
    dropped record has length 0) and ``qual_off`` None, everything that locates the records in the FASTQ text as it
    was; ``totals``: the int64[8] device tensor of ``gf_pp_filter_device``.  ``reasons``: the uint8 device tensor of
    every record's reason follows (R1's, then R2's)."""
    import torch
    need_read_filter(config)
    if config is None:
        raise ValueError("filter_reads_device needs a ReadFilter")
    sides = [batch] + ([mate] if mate is not None else [])
    n = int(batch.n_records)
    for b in sides:
        if b.qual_off is not None:
            raise ValueError("filter_reads_device takes the full FASTQ cut: the qualities at the bases' offsets")
        _lib.need_device_tensors("filter_reads_device", b.bases, b.quals, b.offsets)
        assert b.bases.dtype == torch.uint8 and b.quals.dtype == torch.uint8 and b.offsets.dtype == torch.int64
        assert b.bases.is_contiguous() and b.quals.is_contiguous() and b.offsets.is_contiguous()
        assert int(b.n_records) == n and b.offsets.numel() >= n + 1 and b.quals.numel() >= b.bases.numel()
    L = lib()
    dev = batch.bases.device
    ws_bytes = int(L.gf_pp_workspace_bytes(n))
    ws = _lib.workspace(ws_bytes, dev, stream)
    totals = torch.zeros(8, dtype=torch.int64, device=dev)
    why = torch.zeros(max(n * len(sides), 1), dtype=torch.uint8, device=dev)
    out = [(torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.empty(max(b.bases.numel(), 1), dtype=torch.uint8, device=dev),
            torch.zeros(n + 1, dtype=torch.int64, device=dev)) for b in sides]
    # (records without a base: an empty tensor has no address, and the library wants one with records)
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    ptrs = [[(t if t.numel() else nothing).data_ptr() for t in (b.bases, b.quals)] + [b.offsets.data_ptr()]
            for b in sides] + ([[None] * 3] if mate is None else [])
    outs = [[t.data_ptr() for t in o] for o in out] + ([[None] * 3] if mate is None else [])
    settings = GfPpSettings(*astuple(config))
    check(L.gf_pp_filter_device(indexer._handle(), C.byref(settings), *ptrs[0], *ptrs[1], n, ws.data_ptr(), ws_bytes,
                                *outs[0], *outs[1], why.data_ptr(), totals.data_ptr(), _lib.stream_handle(dev, stream)))
    for t in [x for o in out for x in o] + [totals, why]:
        _lib.for_stream(t, stream)
    new = []
    for b, (ob, oq, off) in zip(sides, out):
        # (the kept bytes are known on the device only: the tensors keep the input's size, the offsets say what counts)
        new.append(b._replace(bases=ob[:b.bases.numel()], quals=oq[:b.bases.numel()], offsets=off, qual_off=None))
    return (*new, totals, why[:n * len(sides)]) if reasons else (*new, totals)


def totals_counters(totals) -> dict:
    """The seven counters of a filter's totals (a sequence of eight integers), under the keys a filtered scan reports."""
    return dict(zip(COUNTER_KEYS, (int(x) for x in list(totals)[1:])))
