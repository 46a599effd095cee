"""The outputs of K scans and their names, handed to the host as one block: ``gf_pk_pack_device`` of libgfpack.so
(include/gf_scan_pack.h).

``PairScan.download()`` makes four synchronous copies and ``HitNames.download()`` three more.  A host that scans one chunk
of reads against K indexes (multi_csv_scan.py, streamed) would make 7 K small copies per chunk, with the device idle
behind them.  Here the K results are packed on the device — the counts never leave it — and fetched with two copies:
the headers, then exactly the bytes that are there.  libgfpack.so is a library of its own next to libgfmatch.so
(genefuserust_amd/scan_csrc/); it is loaded after ``_lib.lib()``.  No CPU fallback: without the libraries and a GPU
``pack_scans_device`` raises; ``unpack_block`` is plain numpy.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import GF_ERR_ARG, GfError
from .hit_names import HitNames
from .read_pair import PairScan

PK_LIB_PATH = os.path.join(_lib._HERE, "libgfpack.so")
MAX_SCANS = 1024
OVER_RETRY, OVER_HITS, OVER_NAMES, BAD_SCAN = 1, 2, 4, 8   # the bits of a scan's header

_vp, _i64 = C.c_void_p, C.c_int64
# libgfpack.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfpack.so links against.
lib, check = _lib.companion(PK_LIB_PATH, "scan pack", "gf_pk_last_error", {
    "gf_pk_block_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "gf_pk_workspace_bytes": (_i64, [_i64]),
    "gf_pk_pack_device": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "gf_pk_last_error": (C.c_char_p, []),
})

# gf_pk_scan: seven pointers (hits, bases, quals, totals, names, name offsets, name totals), three capacities
SCAN_DTYPE = np.dtype([(n, "<u8") for n in ("hits", "bases", "quals", "totals", "names", "name_off", "name_totals")]
                      + [(n, "<i8") for n in ("hits_cap", "bytes_cap", "names_cap")])
assert SCAN_DTYPE.itemsize == 80


def header_bytes(k: int) -> int:
    return 64 * (k + 1)


class UnpackedScan(NamedTuple):
    """One scan of a block: what ``PairScan.download()`` gives (``rec``, ``bases``, ``quals``, ``totals``) and what
    ``HitNames.download()`` gives (``names``); ``bits``: the scan's OVER_* bits — with any set the scan was packed as
    empty, and ``totals["hits"]`` is still its true hit count; ``name_bytes``: the bytes its names take; ``missing``:
    records without a name line."""
    rec: np.ndarray
    bases: bytes
    quals: bytes
    totals: dict
    names: List[bytes]
    bits: int
    name_bytes: int
    missing: int


def unpack_block(block, k: int) -> List[UnpackedScan]:
    """The K scans of a block (bytes, or a uint8 array: the headers and the body).  Raises ``ValueError`` for a block
    that is not one of K scans, that overflowed, or that is shorter than its header says."""
    buf = np.frombuffer(bytes(block), dtype=np.uint8)
    hb = header_bytes(k)
    if buf.size < hb:
        raise ValueError("a block of %d scans has %d bytes of headers, not %d" % (k, hb, buf.size))
    head = buf[:hb].view("<i8").reshape(k + 1, 8)
    body_bytes, kk, over = (int(x) for x in head[0, :3])
    if kk != k:
        raise ValueError("a block of %d scans, not %d" % (kk, k))
    if over:
        raise ValueError("the block overflowed: it takes %d bytes" % (hb + body_bytes))
    if buf.size < hb + body_bytes:
        raise ValueError("the block's body takes %d bytes, %d are here" % (body_bytes, buf.size - hb))
    body = buf[hb:hb + body_bytes]
    scans = head[1:]
    rec_n, rb, nb = scans[:, 0], scans[:, 1], scans[:, 2]
    bits = scans[:, 7] & 255
    # the five sections: per scan the bytes of its part; a section starts on the next 16-byte boundary
    parts = [64 * rec_n, rb, rb, np.where(bits != 0, 0, 8 * (rec_n + 1)), nb]
    at, starts = 0, []
    for p in parts:
        starts.append(at + np.concatenate(([0], np.cumsum(p)[:-1])))
        at = (at + int(p.sum()) + 15) & ~15
    if at != body_bytes:
        raise ValueError("the scans' headers add up to %d bytes of body, the block's says %d" % (at, body_bytes))
    out = []
    for i in range(k):
        cut = [body[int(s[i]):int(s[i]) + int(p[i])] for s, p in zip(starts, parts)]
        off = cut[3].view("<i8")
        names = cut[4].tobytes()
        tot = {"hits": int(scans[i, 5]), "hit_bytes": int(rb[i]), "merged_pairs": int(scans[i, 3]),
               "retried_reads": int(scans[i, 4]), "overflow": int(bits[i])}
        out.append(UnpackedScan(cut[0].view(_lib.PAIR_HIT_DTYPE).reshape(-1).copy(), cut[1].tobytes(), cut[2].tobytes(),
                                tot, [names[off[j]:off[j + 1]] for j in range(int(rec_n[i]))], int(bits[i]),
                                int(scans[i, 7]) >> 8, int(scans[i, 6])))
    return out


def _to_host(t) -> np.ndarray:
    """One synchronous device-to-host copy: every byte ``PackedScans.download`` fetches comes through here."""
    return t.cpu().numpy()


class PackedScans(NamedTuple):
    """What gf_pk_pack_device leaves in HBM: ``block`` uint8[block_bytes], of ``k`` scans; the ``scans`` and ``names``
    it was made from travel with it (the block is packed again from them when it was too small)."""
    block: "object"
    k: int
    scans: Sequence[PairScan]
    names: Sequence[HitNames]
    stream: Optional[int]

    def download(self) -> List[UnpackedScan]:
        """Synchronises.  Two copies — the headers, then exactly the body — and ``unpack_block``.  A block that was too
        small for what the scans hold is packed once more with the size its header asks for (two more copies)."""
        hb = header_bytes(self.k)
        head = _to_host(self.block[:hb])
        body_bytes, _, over = (int(x) for x in head[:24].view("<i8"))
        if over:
            again = pack_scans_device(self.scans, self.names, self.stream, block_bytes=hb + body_bytes)
            head = _to_host(again.block[:hb])
            if int(head[16:24].view("<i8")[0]):
                raise GfError(_lib.GF_ERR_CAPACITY, "a block of the size its header asked for overflowed")
            return unpack_block(np.concatenate((head, _to_host(again.block[hb:hb + body_bytes]))), self.k)
        body = _to_host(self.block[hb:hb + body_bytes]) if body_bytes else np.empty(0, dtype=np.uint8)
        return unpack_block(np.concatenate((head, body)), self.k)


def scan_descriptors(scans: Sequence[PairScan], names: Sequence[HitNames]) -> np.ndarray:
    """The ``gf_pk_scan`` array of K scans and their names (SCAN_DTYPE), as it is uploaded."""
    d = np.zeros(len(scans), dtype=SCAN_DTYPE)
    for i, (s, n) in enumerate(zip(scans, names)):
        d[i] = (s.hits.data_ptr(), s.bases.data_ptr(), s.quals.data_ptr(), s.totals.data_ptr(), n.names.data_ptr(),
                n.offsets.data_ptr(), n.totals.data_ptr(), s.hits.shape[0], min(s.bases.numel(), s.quals.numel()),
                n.names.numel())
    return d


def default_block_bytes(scans: Sequence[PairScan], names: Sequence[HitNames]) -> int:
    """A block for 256 records a scan with 512 bytes of read and 64 of name each — or, where that is less, for what the
    scans' capacities can hold at all."""
    L, k = lib(), len(scans)
    cap = L.gf_pk_block_bytes(k, sum(int(s.hits.shape[0]) for s in scans), sum(int(s.bases.numel()) for s in scans),
                              sum(int(n.names.numel()) for n in names))
    return int(min(cap, L.gf_pk_block_bytes(k, 256 * k, 256 * 512 * k, 256 * 64 * k)))


def pack_scans_device(scans: Sequence[PairScan], names: Sequence[HitNames], stream=None,
                      block_bytes: Optional[int] = None) -> PackedScans:
    """The block of the K ``scans`` and their ``names`` (``hit_names_device`` of each), asynchronously: the descriptors
    are uploaded and gf_pk_pack_device is queued; nothing waits for the scans.  ``block_bytes``: the block's size
    (default: ``default_block_bytes``); a block that turns out too small says so in its header, and ``download`` packs
    it again."""
    import torch
    k = len(scans)
    if not 1 <= k <= MAX_SCANS or len(names) != k:
        raise GfError(GF_ERR_ARG, "pack_scans_device takes 1 .. %d scans and as many names, not %d and %d"
                      % (MAX_SCANS, k, len(names)))
    tensors = [t for s, n in zip(scans, names) for t in (s.hits, s.bases, s.quals, s.totals, n.names, n.offsets, n.totals)]
    _lib.need_device_tensors("pack_scans_device", *tensors)
    for s, n in zip(scans, names):
        assert s.hits.dtype == torch.uint8 and s.hits.is_contiguous() and s.hits.shape[1:] == (64,)
        assert s.totals.dtype == torch.int64 and s.totals.numel() >= 8 and s.totals.is_contiguous()
        assert n.totals.dtype == torch.int64 and n.totals.numel() >= 4 and n.totals.is_contiguous()
        assert n.offsets.dtype == torch.int64 and n.offsets.numel() >= s.hits.shape[0] + 1 and n.offsets.is_contiguous()
        for t in (s.bases, s.quals, n.names):
            assert t.dtype == torch.uint8 and t.is_contiguous()
    L = lib()
    dev = scans[0].totals.device
    block_bytes = default_block_bytes(scans, names) if block_bytes is None else int(block_bytes)
    desc = torch.from_numpy(scan_descriptors(scans, names).view(np.uint8))
    ws_bytes = int(L.gf_pk_workspace_bytes(k))
    ws = _lib.workspace(ws_bytes, dev, stream)
    block = _lib.workspace(block_bytes, dev, stream)
    with torch.cuda.stream(torch.cuda.current_stream(dev) if stream is None
                           else torch.cuda.ExternalStream(stream, device=dev)):
        d_desc = _lib.for_stream(desc.to(dev, non_blocking=True), stream)
    check(L.gf_pk_pack_device(d_desc.data_ptr(), k, ws.data_ptr(), ws_bytes, block.data_ptr(), block_bytes,
                              _lib.stream_handle(dev, stream)))
    return PackedScans(block, k, tuple(scans), tuple(names), stream)
