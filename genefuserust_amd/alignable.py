"""The whole-genome alignable filter, working and on the device: libgfalign.so (include/gf_alignable.h) and the host
side that drives it.  Opt-in (``scan.finish_matches(alignable_filter="genome")``); the reference's own last filter, as
it is, stays in matcher.py (``remove_alignables``) and removes nothing.

The predicate.  Reference: name -> bytes, upper-cased.  Read: bytes, compared as they are; its two
strands are the read and ``fusion_mapper.reverse_complement`` of it.  For a strand ``s`` of length ``L``, a contig ``c``
and a start ``p`` with ``0 <= p`` and ``p + L <= len(c)``, position ``i`` matches when ``s[i] == c[p + i]`` and that
byte is one of ACGT, and is covered when it lies in a window of 16 positions that all match.  A read is alignable when
for either strand, some contig and some ``p`` fewer than 10 positions are uncovered.  A read shorter than 16 never is,
and an alignment never spans two contigs.

    reads  --gf_al_seeds_device-->  both strands, a seed per valid 16-mer, a membership filter over the keys
           --torch.sort-->          the seeds in key order
           --gf_al_index_device-->  where each bucket of keys starts
    reference, piece by piece from pinned staging, the next upload behind the current scan
           --gf_al_scan_device-->   the bit of every read that is alignable in the piece, ORed into the flags

No CPU fallback: without the library and a GPU the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterator, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib

AL_LIB_PATH = os.path.join(_lib._HERE, "libgfalign.so")

K, LIMIT = 16, 10
READS_MAX = 1 << 18
FILTER_LOG2_MIN, FILTER_LOG2_MAX = 16, 32
FILTER_LOG2_DEFAULT = 25     # 2^25 bits = 4 MiB, an XCD's L2: the fastest of 22 .. 32 in profiles/alignable_bench.json
SEPARATOR = 0
FILTERS = (None, "genome")

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
# libgfalign.so, loaded (once) after libgfmatch.so
lib, check = _lib.companion(AL_LIB_PATH, "device alignable filter", "gf_al_last_error", {
    "gf_al_filter_bytes": (_i64, [_i32]),
    "gf_al_bucket_bytes": (_i64, []),
    "gf_al_flag_bytes": (_i64, [_i64]),
    "gf_al_seeds_device": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp]),
    "gf_al_index_device": (C.c_int, [_vp, _i64, _vp, _vp]),
    "gf_al_scan_device": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp]),
    "gf_al_last_error": (C.c_char_p, []),
})


def need_filter(alignable_filter, remove_alignables: bool = False) -> bool:
    """Whether ``alignable_filter`` names the genome filter; ``ValueError`` for anything but None and "genome", and for
    the genome filter together with ``remove_alignables`` (the as-is mirror: one last filter, not two)."""
    if alignable_filter not in FILTERS:
        raise ValueError("alignable_filter must be None or 'genome', not %r" % (alignable_filter,))
    if alignable_filter is not None and remove_alignables:
        raise ValueError("alignable_filter=%r and remove_alignables=True are two forms of one filter: give one"
                         % (alignable_filter,))
    return alignable_filter is not None


def plan_pieces(lengths: Sequence[int], piece_bytes: int, overlap: int) -> List[List[Tuple[int, int, int]]]:
    """The pieces of a reference whose contigs have ``lengths``: each a list of (contig, start, end) parts, one
    separator byte between two parts.  A contig that fits shares a piece with its neighbours; one longer than
    ``piece_bytes`` is cut into pieces that overlap by ``overlap`` bases, so that every stretch of ``overlap + 1`` bases
    of it lies whole in one piece.  ``piece_bytes > overlap``."""
    assert piece_bytes > overlap >= 0
    pieces: List[List[Tuple[int, int, int]]] = []
    cur: List[Tuple[int, int, int]] = []
    room = piece_bytes
    for k, n in enumerate(lengths):
        n = int(n)
        if n == 0:
            continue
        start = 0
        while n - start > piece_bytes:   # (a long contig: whole pieces of its own)
            if cur:
                pieces.append(cur)
                cur, room = [], piece_bytes
            pieces.append([(k, start, start + piece_bytes)])
            start += piece_bytes - overlap
        need = n - start + (1 if cur else 0)
        if need > room:
            pieces.append(cur)
            cur, room, need = [], piece_bytes, n - start
        cur.append((k, start, n))
        room -= need
    if cur:
        pieces.append(cur)
    return pieces


def _fill_piece(out: np.ndarray, parts, contigs: Sequence[np.ndarray]) -> int:
    """The text of a piece into ``out``; its length."""
    at = 0
    for i, (k, s, e) in enumerate(parts):
        if i:
            out[at] = SEPARATOR
            at += 1
        out[at:at + e - s] = contigs[k][s:e]
        at += e - s
    return at


def _torch_device(device):
    import torch
    if isinstance(device, torch.device):
        return device
    if not torch.cuda.is_available():
        raise _lib.GfError(_lib.GF_ERR_NO_DEVICE, "the device alignable filter needs a GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device() if device is None or int(device) < 0 else int(device))


def _batches(n: int) -> Iterator[Tuple[int, int]]:
    for a in range(0, n, READS_MAX):
        yield a, min(n, a + READS_MAX)


def alignable_reads_device(reference: Optional[Mapping[str, bytes]], reads: Sequence[bytes], device=-1,
                           batch_bytes: int = 256 << 20, *, filter_log2_bits: int = None,
                           stats: dict = None) -> np.ndarray:
    """bool[len(reads)]: whether each read is alignable in ``reference`` (name -> bytes), by the predicate at the top.

    The reference is uploaded piece by piece from pinned staging, the next upload behind the current scan; a piece has
    ``batch_bytes`` bytes, and never fewer than twice the longest read.  Small contigs share a piece; a contig longer
    than a piece is cut into pieces that overlap by the longest read less one base.  The result does not depend on
    ``batch_bytes``.  With no reads nothing is uploaded; with ``reference`` None or empty nothing is alignable
    (fusion_mapper.rs:489-491).  A read longer than ``GF_MAX_READ_LEN`` raises ``GfError``.

    ``filter_log2_bits``: the membership filter has 2 to that many bits (16 .. 32; 32: the exact map of all keys); the
    result does not depend on it.  ``stats`` (a dict): gets ``scan_ms`` (the scan kernels' time from device events, one
    per piece), ``text_bytes``, ``pieces`` and ``seeds``."""
    reads = [bytes(r) for r in reads]
    flags = np.zeros(len(reads), dtype=bool)
    log2_bits = FILTER_LOG2_DEFAULT if filter_log2_bits is None else int(filter_log2_bits)
    if not FILTER_LOG2_MIN <= log2_bits <= FILTER_LOG2_MAX:
        raise ValueError("filter_log2_bits must be %d .. %d, not %r" % (FILTER_LOG2_MIN, FILTER_LOG2_MAX, filter_log2_bits))
    if int(batch_bytes) < 1:
        raise ValueError("batch_bytes must be positive, not %r" % (batch_bytes,))
    longest = max((len(r) for r in reads), default=0)
    if longest > _lib.GF_MAX_READ_LEN:
        raise _lib.GfError(_lib.GF_ERR_READ_TOO_LONG, "a read of %d bases: the alignable filter takes up to %d"
                           % (longest, _lib.GF_MAX_READ_LEN))
    if stats is not None:
        stats.update(scan_ms=[], text_bytes=0, pieces=0, seeds=0)
    if not reads or not reference or longest < K:
        return flags
    import torch
    dev = _torch_device(device)
    contigs = [np.frombuffer(c if isinstance(c, (bytes, bytearray, memoryview)) else bytes(c), dtype=np.uint8)
               for c in reference.values()]
    # (no larger than the whole reference with its separators: the staging buffers have a piece's size)
    piece_bytes = max(min(int(batch_bytes), sum(c.size for c in contigs) + len(contigs)), 2 * longest)
    piece_bytes += -piece_bytes % 16
    pieces = plan_pieces([c.size for c in contigs], piece_bytes, longest - 1)
    if not pieces:
        return flags
    L = lib()
    with torch.cuda.device(dev):
        main = torch.cuda.current_stream(dev)
        copy = torch.cuda.Stream(dev)
        staging = [torch.empty(piece_bytes, dtype=torch.uint8).pin_memory() for _ in range(min(2, len(pieces)))]
        text = [torch.empty(piece_bytes, dtype=torch.uint8, device=dev) for _ in staging]
        uploaded = [torch.cuda.Event() for _ in staging]
        scanned = [torch.cuda.Event() for _ in staging]
        timers = []
        for a, b in _batches(len(reads)):
            lengths = np.fromiter((len(r) for r in reads[a:b]), dtype=np.int64, count=b - a)
            offsets = np.zeros(b - a + 1, dtype=np.int64)
            np.cumsum(lengths, out=offsets[1:])
            n_bases = int(offsets[-1])
            if n_bases == 0:
                continue
            d_bases = torch.from_numpy(np.frombuffer(b"".join(reads[a:b]), dtype=np.uint8).copy()).to(dev)
            d_offsets = torch.from_numpy(offsets).to(dev)
            d_strands = torch.empty(2 * n_bases, dtype=torch.uint8, device=dev)
            d_seeds = torch.empty(2 * n_bases, dtype=torch.int64, device=dev)
            d_filter = torch.empty(L.gf_al_filter_bytes(log2_bits), dtype=torch.uint8, device=dev)
            d_buckets = torch.empty(L.gf_al_bucket_bytes() // 4, dtype=torch.int32, device=dev)
            d_flags = torch.zeros(L.gf_al_flag_bytes(b - a) // 4, dtype=torch.int32, device=dev)
            check(L.gf_al_seeds_device(d_bases.data_ptr(), n_bases, d_offsets.data_ptr(), b - a, d_strands.data_ptr(),
                                       d_seeds.data_ptr(), d_filter.data_ptr(), log2_bits, main.cuda_stream))
            d_seeds = torch.sort(d_seeds).values   # (plumbing: the slots without a seed are INT64_MAX and sort last)
            check(L.gf_al_index_device(d_seeds.data_ptr(), 2 * n_bases, d_buckets.data_ptr(), main.cuda_stream))
            if stats is not None:
                stats["seeds"] += int((d_seeds != np.iinfo(np.int64).max).sum())
            for k, parts in enumerate(pieces):
                slot = k % len(staging)
                # the scan that last read this slot's text is done: its staging buffer was uploaded before it started
                scanned[slot].synchronize()
                n = _fill_piece(staging[slot].numpy(), parts, contigs)
                with torch.cuda.stream(copy):
                    text[slot][:n].copy_(staging[slot][:n], non_blocking=True)
                    uploaded[slot].record(copy)
                main.wait_event(uploaded[slot])
                if stats is not None:
                    timers.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                    timers[-1][0].record(main)
                check(L.gf_al_scan_device(text[slot].data_ptr(), n, d_strands.data_ptr(), n_bases, d_offsets.data_ptr(),
                                          b - a, d_seeds.data_ptr(), d_buckets.data_ptr(), d_filter.data_ptr(),
                                          log2_bits, d_flags.data_ptr(), main.cuda_stream))
                if stats is not None:
                    timers[-1][1].record(main)
                    stats["text_bytes"] += n
                    stats["pieces"] += 1
                scanned[slot].record(main)
            words = d_flags.cpu().numpy().view(np.uint32)
            flags[a:b] = (words[np.arange(b - a) >> 5] >> (np.arange(b - a) & 31).astype(np.uint32)) & 1 != 0
        main.synchronize()
        if stats is not None:
            stats["scan_ms"] = [t0.elapsed_time(t1) for t0, t1 in timers]
    return flags


def remove_genome_alignables(matches: Sequence, reference, device=-1):
    """(the matches whose read is not alignable in ``reference``, how many were dropped): one
    ``alignable_reads_device`` call for all of them."""
    if not matches:
        return list(matches), 0
    drop = alignable_reads_device(reference, [bytes(m.m_read) for m in matches], device)
    return [m for m, d in zip(matches, drop.tolist()) if not d], int(drop.sum())
