"""Bases inside the overlap of a pair corrected from the mate on the device, opt-in: ``gf_oc_correct_device`` of
libgfcorrect.so (include/gf_overlap_correct.h).

Where the mates of a pair overlap, a base is read twice.  A poor call that a confident call of the mate contradicts is
a miscall: ``fast_merge`` tolerates two of them in the overlap and maps a pair with three as two separate mates, the
duplicate removal keys on the exact bases and counts PCR copies that differ by one of them as two molecules, and the
cleaned reads carry them to the aligner.  Here they are rewritten while the records sit in HBM between the FASTQ cut
and the adapter trimming: the overlap is found as the trimming finds it (the largest accepted insert length), and at
every difference inside it the base of ``bad_phred`` or less takes the complement and the quality of the mate's base
of ``good_phred`` or more.  Lengths, offsets, the record count and order stay, so the names and the original records
of a scan's matches are gathered from the FASTQ text as before.  A feature outside the reference, off unless an
``OverlapCorrect`` is handed to a route.  libgfcorrect.so is a library of its own on top of libgfmatch.so's public C
ABI (genefuserust_amd/scan_csrc/).  No CPU fallback: without the libraries and a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

from . import _lib

OC_LIB_PATH = os.path.join(_lib._HERE, "libgfcorrect.so")

READ_MAX, PHRED_MAX, TOTALS = 512, 93, 6
# the keys the totals of a corrected scan go by, behind "pairs seen" (which ``pairs`` already counts)
CORRECT_COUNTER_KEYS = ("correction_overlapping_pairs", "correction_pairs_with_diffs", "corrected_reads",
                        "corrected_bases", "correction_diffs_left")


@dataclass(frozen=True)
class OverlapCorrect:
    """The settings of the correction (include/gf_overlap_correct.h says what it does).  ``ValueError`` for what the
    library refuses: ``min_overlap`` outside 8 .. 512, a negative ``max_diff``, ``diff_percent`` outside 0 .. 100,
    ``good_phred`` or ``bad_phred`` outside 0 .. 93, and ``bad_phred`` not below ``good_phred``."""
    min_overlap: int = 30        # the fewest positions an accepted insert compares
    max_diff: int = 5            # the most differences of an accepted insert
    diff_percent: int = 20       # the share of differences of an accepted insert
    good_phred: int = 30         # a source's phred is at least this (fast_merge's '?')
    bad_phred: int = 15          # a corrected base's phred is at most this (fast_merge's '0')

    def __post_init__(self):
        limits = dict(min_overlap=(8, READ_MAX), max_diff=(0, 2 ** 31 - 1), diff_percent=(0, 100),
                      good_phred=(0, PHRED_MAX), bad_phred=(0, PHRED_MAX))
        for name, (lo, hi) in limits.items():
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError("OverlapCorrect.%s must be an integer in %d .. %d, not %r" % (name, lo, hi, v))
        if self.bad_phred >= self.good_phred:
            raise ValueError("OverlapCorrect.bad_phred must be below good_phred, not %d against %d"
                             % (self.bad_phred, self.good_phred))


def need_overlap_correct(x) -> Optional[OverlapCorrect]:
    """``x`` when it is None or an ``OverlapCorrect``; ``ValueError`` for anything else."""
    if x is None or isinstance(x, OverlapCorrect):
        return x
    raise ValueError("overlap_correct must be None or an OverlapCorrect, not %r" % (x,))


def need_pairs(x, paired: bool) -> Optional[OverlapCorrect]:
    """``need_overlap_correct``, and ``ValueError`` for an ``OverlapCorrect`` with single-end input."""
    if need_overlap_correct(x) is not None and not paired:
        raise ValueError("overlap_correct: the correction needs pairs, and this input is single-end")
    return x


class GfOcSettings(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ("min_overlap", "max_diff", "diff_percent", "good_phred", "bad_phred")]


def settings_of(config: OverlapCorrect) -> GfOcSettings:
    """The library's struct for ``config``."""
    return GfOcSettings(config.min_overlap, config.max_diff, config.diff_percent, config.good_phred, config.bad_phred)


_vp, _i64 = C.c_void_p, C.c_int64
# libgfcorrect.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfcorrect.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(OC_LIB_PATH, "overlap correction", "gf_oc_last_error", {
    "gf_oc_correct_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "gf_oc_last_error": (C.c_char_p, []),
})


def correct_overlaps_device(indexer, config: OverlapCorrect, batch, mate, stream=None, detail: bool = False,
                            inplace: bool = False):
    """The correction over the pairs of ``batch`` and ``mate`` (``FastqBatch``es of the full cut: the qualities at the
    bases' offsets), record by record, asynchronously, in one call.  Returns (batch, mate, totals): the batches with
    ``bases`` and ``quals`` corrected and everything else — the offsets, and what locates the records in the FASTQ
    text — as it was; ``totals``: the int64[6] device tensor of ``gf_oc_correct_device``.  ``detail``: ``insert``
    (int32[n], I* of every pair or -1) and ``fixed`` (int32[2 n], the bases corrected in each R1, then in each R2)
    follow.  ``inplace=False`` (the default): bases and qualities are cloned on the stream first and the clones are
    corrected, so the batches handed in stay byte for byte; ``inplace=True``: their own tensors are rewritten and
    returned.  ``ValueError`` without a mate, without a config, and for batches of the lean cut."""
    import torch
    need_overlap_correct(config)
    if config is None:
        raise ValueError("correct_overlaps_device needs an OverlapCorrect")
    if mate is None:
        raise ValueError("correct_overlaps_device: the correction needs pairs, and there is no mate")
    sides = [batch, mate]
    n = int(batch.n_records)
    for b in sides:
        if b.qual_off is not None:
            raise ValueError("correct_overlaps_device takes the full FASTQ cut: the qualities at the bases' offsets")
        _lib.need_device_tensors("correct_overlaps_device", b.bases, b.quals, b.offsets)
        assert b.bases.dtype == torch.uint8 and b.quals.dtype == torch.uint8 and b.offsets.dtype == torch.int64
        assert b.bases.is_contiguous() and b.quals.is_contiguous() and b.offsets.is_contiguous()
        assert int(b.n_records) == n and b.offsets.numel() >= n + 1 and b.quals.numel() >= b.bases.numel()
    L = lib()
    dev = batch.bases.device
    handle = _lib.stream_handle(dev, stream)
    if not inplace:
        clones = lambda: [b._replace(bases=b.bases.clone(), quals=b.quals.clone()) for b in sides]   # noqa: E731
        if stream is None:
            sides = clones()
        else:
            with torch.cuda.stream(torch.cuda.ExternalStream(stream, device=dev)):
                sides = clones()
    totals = torch.zeros(TOTALS, dtype=torch.int64, device=dev)
    insert = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if detail else None
    fixed = torch.empty(max(2 * n, 1), dtype=torch.int32, device=dev) if detail else None
    # (records without a base: an empty tensor has no address, and the library wants one with records)
    nothing = torch.zeros(16, dtype=torch.uint8, device=dev)
    ptrs = [[(t if t.numel() else nothing).data_ptr() for t in (b.bases, b.quals)] + [b.offsets.data_ptr()]
            for b in sides]
    settings = settings_of(config)
    check(L.gf_oc_correct_device(indexer._handle(), C.byref(settings), *ptrs[0], *ptrs[1], n,
                                 insert.data_ptr() if detail else None, fixed.data_ptr() if detail else None,
                                 totals.data_ptr(), handle))
    for t in [x for b in sides for x in (b.bases, b.quals)] + [totals] + ([insert, fixed] if detail else []):
        _lib.for_stream(t, stream)
    return (*sides, totals, insert[:n], fixed[:2 * n]) if detail else (*sides, totals)


def correct_totals_counters(totals) -> dict:
    """The five counters of a correction's totals (a sequence of six integers), under the keys a corrected scan
    reports."""
    return dict(zip(CORRECT_COUNTER_KEYS, (int(x) for x in list(totals)[1:])))
