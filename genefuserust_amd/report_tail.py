"""The report tail in bulk: libgfreport.so (include/gf_report.h) and the host side that drives it.

Every scan route ends in ``scan.finish_matches`` and ``scan.report_matches``: the three filters of
``FusionMapper.filter_matches``, ``sort_matches``, the first-fit clustering of ``fusion_result.cluster_matches`` and
``adjust_fusion_break``.  On the host that is one library call per match in the filter, one per comparison in the sort
and 28 per match in the break refinement, and a first fit that scans every match of every cluster.  With
``tail="device"`` the same steps run over all matches at once:

    matches  --MatchTable-->  bases blob + offsets + gf_readmatch[n]
        --gf_rp_filter_device-->  a reason per match                              (``filter_reasons_device``)
        --numpy.lexsort-->  the order of ``sort_matches``                         (``order_matches``, host)
        --gf_rp_first_fit-->  the founder of each match's cluster, O(49 n)        (``first_fit``, host, no GPU)
        --gf_rp_adjust_device-->  {shift, left distance, right distance} per match, all clusters in one call
                                                                                  (``adjust_breaks_device``)

Everything between those steps — ``calc_fusion_point``, ``make_reference``, ``calc_unique``, ``update_info``,
``is_qualified``, the final sort — is ``fusion_result.cluster_with``, the body ``cluster_matches`` runs too.  Results,
counters and report bytes are those of the host tail.  No CPU fallback: without the library and a GPU the device calls
raise; ``first_fit`` and ``order_matches`` need neither.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, NamedTuple, Sequence

import numpy as np

from . import _lib
from ._lib import READMATCH_DTYPE
from .fusion_mapper import FusionMapper, ReadMatch
from .fusion_result import FusionResult, Settings, cluster_with

RP_LIB_PATH = os.path.join(_lib._HERE, "libgfreport.so")

STATUS_OK, STATUS_OUT_OF_DOMAIN, STATUS_BAD_ROW = 0, 1, 2
REASON_BAD_BREAK, REASON_BAD_READ = -1, -2
TAILS = ("host", "device")

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
# libgfreport.so, loaded (once) after libgfmatch.so
lib, check = _lib.companion(RP_LIB_PATH, "device report tail", "gf_rp_last_error", {
    "gf_rp_filter_device": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp]),
    "gf_rp_adjust_device": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    "gf_rp_first_fit": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "gf_rp_last_error": (C.c_char_p, []),
})


def need_tail(tail: str) -> bool:
    """Whether ``tail`` names the device tail; ``ValueError`` for anything but "host" and "device"."""
    if tail not in TAILS:
        raise ValueError("tail must be 'host' or 'device', not %r" % (tail,))
    return tail == "device"


class MatchTable(NamedTuple):
    """Matches as arrays: the reads back to back in ``bases`` (uint8), read i at ``offsets[i]:offsets[i + 1]`` (int64
    [n + 1]), ``rm`` a ``READMATCH_DTYPE`` array, ``lengths`` the reads' lengths (int64)."""
    bases: np.ndarray
    offsets: np.ndarray
    rm: np.ndarray
    lengths: np.ndarray

    @classmethod
    def from_matches(cls, matches: Sequence[ReadMatch]) -> "MatchTable":
        n = len(matches)
        lengths = np.fromiter((len(m.m_read) for m in matches), dtype=np.int64, count=n)
        offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lengths, out=offsets[1:])
        bases = np.frombuffer(b"".join(bytes(m.m_read) for m in matches), dtype=np.uint8)
        rm = np.zeros(n, dtype=READMATCH_DTYPE)
        for field, get in (
                ("read_break", lambda m: m.m_read_break), ("gap", lambda m: m.m_gap),
                ("left_distance", lambda m: m.m_left_distance), ("right_distance", lambda m: m.m_right_distance),
                ("left_position", lambda m: m.m_left_gp.position), ("right_position", lambda m: m.m_right_gp.position),
                ("left_contig", lambda m: m.m_left_gp.contig), ("right_contig", lambda m: m.m_right_gp.contig)):
            rm[field] = np.fromiter((get(m) for m in matches), dtype=np.int64, count=n)
        return cls(bases, offsets, rm, lengths)

    def __len__(self) -> int:   # (of matches, not of fields)
        return int(self.lengths.size)


def _upload(a: np.ndarray, dev):
    """``a``'s bytes as a uint8 device tensor (at least one byte, so that it has an address)."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if raw.size == 0:
        return torch.zeros(1, dtype=torch.uint8, device=dev)
    return torch.from_numpy(raw.copy()).to(dev)


def _torch_device(device):
    import torch
    if isinstance(device, torch.device):
        return device
    if not torch.cuda.is_available():
        raise _lib.GfError(_lib.GF_ERR_NO_DEVICE, "the device report tail needs a GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device() if device is None or int(device) < 0 else int(device))


def filter_reasons_device(table: MatchTable, deletion_threshold: int, device=-1) -> np.ndarray:
    """``gf_readmatch_filter``'s reason per match (int32[n]: 0 kept, 1 complexity, 2 distance, 3 indels; negative: a
    ``read_break`` outside its read), all matches in one ``gf_rp_filter_device`` call."""
    import torch
    n = len(table)
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    dev = _torch_device(device)
    bases, offsets, rm = _upload(table.bases, dev), _upload(table.offsets, dev), _upload(table.rm, dev)
    reason = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib().gf_rp_filter_device(bases.data_ptr(), table.bases.size, offsets.data_ptr(), rm.data_ptr(), n,
                                    int(deletion_threshold), reason.data_ptr(), _lib.stream_handle(dev)))
    return reason.cpu().numpy()


def first_fit(lp, rp, group_off) -> np.ndarray:
    """``gf_rp_first_fit``: per match the index of the match that founded the cluster it joins (int64[n]).  ``lp`` /
    ``rp``: the left and right positions of the matches of all groups, each group in its sorted order; ``group_off``
    [n_groups + 1]: where each group starts.  Host code, no GPU."""
    lp, rp = np.ascontiguousarray(lp, dtype=np.int32), np.ascontiguousarray(rp, dtype=np.int32)
    group_off = np.ascontiguousarray(group_off, dtype=np.int64)
    n_groups = group_off.size - 1
    assert n_groups >= 0 and lp.ndim == rp.ndim == 1 and lp.size == rp.size
    assert n_groups == 0 and lp.size == 0 or group_off[-1] == lp.size
    founder = np.empty(lp.size, dtype=np.int64)
    check(lib().gf_rp_first_fit(lp.ctypes.data if lp.size else None, rp.ctypes.data if rp.size else None,
                                group_off.ctypes.data, n_groups, founder.ctypes.data if founder.size else None))
    return founder


def adjust_breaks_device(table: MatchTable, cluster, refs: np.ndarray, ref_offsets, device=-1) -> np.ndarray:
    """``adjust_fusion_break`` for every match of ``table``, one ``gf_rp_adjust_device`` call: int32[n, 4] =
    (shift, left distance, right distance, status).  ``cluster`` [n]: each match's cluster; ``refs`` (uint8): the
    clusters' references back to back, ``ref_offsets`` [2 * n_clusters + 1]: left then right reference per cluster."""
    import torch
    n = len(table)
    if n == 0:
        return np.zeros((0, 4), dtype=np.int32)
    cluster = np.ascontiguousarray(cluster, dtype=np.int32)
    ref_offsets = np.ascontiguousarray(ref_offsets, dtype=np.int64)
    refs = np.ascontiguousarray(refs, dtype=np.uint8)
    assert cluster.size == n and ref_offsets.size % 2 == 1
    dev = _torch_device(device)
    bases, offsets, rm = _upload(table.bases, dev), _upload(table.offsets, dev), _upload(table.rm, dev)
    d_cluster, d_refs, d_roff = _upload(cluster, dev), _upload(refs, dev), _upload(ref_offsets, dev)
    out = torch.empty((n, 4), dtype=torch.int32, device=dev)
    check(lib().gf_rp_adjust_device(bases.data_ptr(), table.bases.size, offsets.data_ptr(), rm.data_ptr(),
                                    d_cluster.data_ptr(), n, d_refs.data_ptr(), refs.size, d_roff.data_ptr(),
                                    ref_offsets.size // 2, out.data_ptr(), _lib.stream_handle(dev)))
    return out.cpu().numpy()


def order_matches(matches: Sequence[ReadMatch]) -> List[ReadMatch]:
    """``FusionMapper.sort_matches``'s order (read_break descending, shorter read first, name descending; stable): the
    two numeric keys through one ``numpy.lexsort``, the comparator only inside the runs that tie on both."""
    n = len(matches)
    if n < 2:
        return list(matches)
    brk = np.fromiter((m.m_read_break for m in matches), dtype=np.int64, count=n)
    length = np.fromiter((len(m.m_read) for m in matches), dtype=np.int64, count=n)
    order = np.lexsort((length, -brk))   # (stable: a run keeps the matches' own order)
    b, l = brk[order], length[order]
    starts = np.concatenate(([0], np.nonzero((b[1:] != b[:-1]) | (l[1:] != l[:-1]))[0] + 1, [n]))
    out: List[ReadMatch] = []
    for s, e in zip(starts[:-1].tolist(), starts[1:].tolist()):
        run = [matches[k] for k in order[s:e].tolist()]
        out += run if e - s == 1 else FusionMapper.sort_matches(run)
    return out


def _first_fit_bulk(groups: Sequence[Sequence[ReadMatch]]) -> List[FusionResult]:
    """``fusion_result.first_fit_clusters`` through one ``first_fit`` call for all groups."""
    flat = [m for fm in groups for m in fm]
    group_off = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([len(fm) for fm in groups], out=group_off[1:])
    founder = first_fit(np.fromiter((m.m_left_gp.position for m in flat), dtype=np.int32, count=len(flat)),
                        np.fromiter((m.m_right_gp.position for m in flat), dtype=np.int32, count=len(flat)), group_off)
    by_founder: dict = {}   # (insertion order = founder order = the order the clusters are made in)
    for m, f in zip(flat, founder.tolist()):
        fr = by_founder.get(f)
        if fr is None:
            fr = by_founder[f] = FusionResult()
        fr.add_match(m)
    return list(by_founder.values())


def _adjust_bulk(frs: Sequence[FusionResult], device) -> None:
    """``fusion_result.adjust_clusters`` through one ``adjust_breaks_device`` call for all matches of all clusters; a
    match outside the core's domain goes through ``FusionResult.best_shift``."""
    flat = [m for fr in frs for m in fr.m_matches]
    cluster = np.repeat(np.arange(len(frs), dtype=np.int32), [len(fr.m_matches) for fr in frs])
    pieces = [r for fr in frs for r in (fr.m_left_ref, fr.m_right_ref)]
    ref_offsets = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in pieces], out=ref_offsets[1:])
    out = adjust_breaks_device(MatchTable.from_matches(flat), cluster, np.frombuffer(b"".join(pieces), dtype=np.uint8),
                               ref_offsets, device)
    bad = np.nonzero(out[:, 3] == STATUS_BAD_ROW)[0]
    if bad.size:
        raise _lib.GfError(_lib.GF_ERR_ARG, "gf_rp_adjust_device: match %d points outside its arrays" % int(bad[0]))
    k = 0
    for fr in frs:
        adjusted = []
        for m in fr.m_matches:
            shift, ld, rd, status = out[k].tolist()
            adjusted.append(fr.shifted(m, shift, ld, rd) if status == STATUS_OK else fr.shifted(m, *fr.best_shift(m)))
            k += 1
        fr.m_matches = adjusted


def cluster_matches_device(groups: Sequence[Sequence[ReadMatch]], fusions, fusion_seq: Sequence[str],
                           settings: Settings = None, device=-1) -> List[FusionResult]:
    """``fusion_result.cluster_matches``, the same ``FusionResult`` list: the first fit of all groups in one host call,
    the breaks of all matches of all clusters in one device call, every other step by the methods ``cluster_matches``
    uses (``fusion_result.cluster_with``)."""
    return cluster_with(groups, fusions, fusion_seq, settings, _first_fit_bulk, lambda frs: _adjust_bulk(frs, device))


def filter_matches_device(matches: Sequence[ReadMatch], deletion_threshold: int, device=-1):
    """``FusionMapper.filter_matches``: (kept, the three counters), the reasons from ``filter_reasons_device``."""
    reasons = filter_reasons_device(MatchTable.from_matches(matches), deletion_threshold, device)
    bad = np.nonzero(reasons < 0)[0]
    if bad.size:   # (gf_readmatch_filter's error)
        raise _lib.GfError(_lib.GF_ERR_ARG, "read_break outside the read (match %d)" % int(bad[0]))
    counts = np.bincount(reasons, minlength=4)
    removed = {"complexity": int(counts[1]), "distance": int(counts[2]), "indels": int(counts[3])}
    return [m for m, why in zip(matches, reasons.tolist()) if why == 0], removed
