"""``SingleEndScanner::scan_single_end`` (src/core/sescanner.rs:183-205) for a batch of reads resident in HBM, one
asynchronous call: ``gf_se_scan_device`` of libgfse.so (include/gf_single_end.h).

libgfse.so is a library of its own on top of libgfmatch.so's public C ABI (genefuserust_amd/scan_csrc/); it is loaded
after ``_lib.lib()`` so that both refer to the one libgfmatch.so of this tree.  The result is a ``PairScan`` in the
format of ``gf_scan_pairs_device`` (source 1 = "r1"), so ``PairScan.download``, ``finish_pair_hits`` and
``finish_pair_hits_device`` take it unchanged.  No CPU fallback: without the libraries and a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import _lib
from ._lib import GF_ERR_READ_TOO_LONG, GfError
from .indexer import Indexer
from .read_pair import PairScan, companion_scan, gene_reversed_device

SE_LIB_PATH = os.path.join(_lib._HERE, "libgfse.so")

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
# libgfse.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfse.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(SE_LIB_PATH, "single-end scan", "gf_se_last_error", {
    "gf_se_retry_capacity": (_i64, [_i64]),
    "gf_se_workspace_bytes": (_i64, [_i64, _i32, _i64]),
    "gf_se_scan_device": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i32, _i64, _i64, _vp, _i64, _vp, _i64,
                                    _vp, _vp, _i64, _vp, _vp]),
    "gf_se_last_error": (C.c_char_p, []),
})


def scan_single_device(indexer: Indexer, bases, quals, offsets, max_read_len: int, read_id_base: int = 0,
                       hits_cap: Optional[int] = None, bytes_cap: Optional[int] = None, retry_cap: int = 0,
                       stream=None, check_lengths: bool = True) -> PairScan:
    """The single-end policy for the ``n = offsets.numel() - 1`` reads of ``bases`` / ``quals`` (uint8, the layout
    ``fastq_cut_device`` writes) and ``offsets`` (int64[n+1]), all on the index's device: map every read; a read with
    two segments in the wrong direction is searched again as its reverse complement.  One ``gf_pair_hit`` per hit
    (``pair_id = read_id_base + r``, ``source`` 1, ``flags`` 3 on the reverse complement), in read order.

    ``check_lengths``: wait for the totals and raise ``GfError(GF_ERR_READ_TOO_LONG)`` when a read is longer than
    ``max_read_len`` (totals[5]); False leaves the call fully asynchronous and the check to the caller."""
    import torch
    _lib.need_device_tensors("scan_single_device", bases, quals, offsets)
    assert bases.dtype == torch.uint8 and quals.dtype == torch.uint8 and offsets.dtype == torch.int64
    assert quals.numel() >= bases.numel() and offsets.is_contiguous() and bases.is_contiguous() and quals.is_contiguous()
    L = lib()
    n = offsets.numel() - 1
    dev = bases.device
    hits_cap = max(1024, n // 16) if hits_cap is None else int(hits_cap)
    bytes_cap = hits_cap * max(int(max_read_len), 1) if bytes_cap is None else int(bytes_cap)
    ws_bytes = int(L.gf_se_workspace_bytes(n, int(max_read_len), int(retry_cap)))
    head = (indexer._handle(), bases.data_ptr(), quals.data_ptr(), offsets.data_ptr(), bases.numel(), n,
            int(max_read_len), gene_reversed_device(indexer, dev).data_ptr(), len(indexer.m_fusions), int(read_id_base),
            int(retry_cap))
    scan = companion_scan(check, L.gf_se_scan_device, head, dev, ws_bytes, hits_cap, bytes_cap, stream)
    if check_lengths:
        if stream is not None:
            torch.cuda.ExternalStream(stream, device=dev).synchronize()
        too_long = int(scan.totals[5].item())
        if too_long:
            raise GfError(GF_ERR_READ_TOO_LONG, "%d reads are longer than max_read_len = %d" % (too_long, max_read_len))
    return scan
