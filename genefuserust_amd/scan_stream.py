"""The scans as a stream of FASTQ text: ``PairEndScanner::scan`` / ``SingleEndScanner::scan`` read their files in
packs while the consumers map them (src/core/pescanner.rs:255-395, sescanner.rs:62-181); here the host hands over raw
text chunks — any byte boundaries, it does not parse — and everything from the records to the hit
list happens on the device, chunk k+1 being read and crossing the link while chunk k is processed:

    byte source (a file, gunzipped as it is read; a text in memory)  --readinto, upload threads-->  pinned staging
    block  --H2D, copy stream-->  device text buffer (behind the carried-over tail of the previous chunk)  -->
    gf_fastq_index_device / gf_fastq_gather_device  -->  (on request gf_um_cut_device or gf_um_names_device, the UMIs,
    gf_oc_correct_device, the correction inside the pair overlap,
    gf_at_trim_device, the adapter trimming, and
    gf_pp_filter_device, the read filter, and the gf_dd_* calls, the duplicate removal, and gf_rw_format_device, the
    cleaned records as FASTQ text for the output files)  -->
    gf_scan_pairs_device (merge, map, reverse-complement
    retries, ordered compaction) or gf_se_scan_device  -->  gf_hn_names_device (the names of the hit records; on
    request gf_hn_records_device, their whole FASTQ records for the HTML report)  -->
    gf_pair_hit records + their reads + their names, back to the host; gf_pair_hits_finish there.

A chunk ends anywhere; the bytes after its last complete record (of the record count both files
share) are carried to the front of the next chunk on the device.  A few tiny read-backs per chunk
(the line counts, the carry positions) are the only synchronisation before the results.  The loop itself — threads,
staging blocks, streams, carries — is ``chunk_stream.ChunkStream``; here is what a chunk of FASTQ means.  No CPU fallback.
"""
from __future__ import annotations

from contextlib import closing
from functools import partial
from typing import Iterator, List, Optional, Tuple

import numpy as np

from . import _lib
from .chunk_stream import CARRY_MAX, ArraySource, ChunkStream, fill_read_sizes  # noqa: F401  (both re-exported)
from .fusion_mapper import FusionMapper, ReadMatch
from .indexer import Indexer
from .read_pair import finish_pair_hits, scan_pairs_device, scan_with_room


def _record_cuts(batches, texts, final, side_names):
    """(m, counts, cuts): per side how many records its text has, the count ``m`` all sides share, and where each side's
    tail — what is carried to the next chunk — begins."""
    # A side whose last byte has arrived counts its unterminated last line (fastq_reader.rs:75-147); the others only
    # the lines that end inside the chunk.
    counts = [b.n_records if f else b.n_newlines // 4 for b, f in zip(batches, final)]
    m = min(counts)
    cuts = []
    for b, t, name in zip(batches, texts, side_names):
        if m == 0:
            cut = 0
        elif 4 * m - 1 < b.n_newlines:
            cut = int(b.nl_pos[4 * m - 1].item()) + 1
        else:   # record m-1 ends with the text (no final newline)
            cut = t.numel()
        if t.numel() - cut > CARRY_MAX:
            raise _lib.GfError(_lib.GF_ERR_CAPACITY, "%s: a FASTQ chunk left more than %d bytes for the next one: a "
                               "record does not fit, or the two files' records drift apart faster than the chunks "
                               "can absorb" % (name, CARRY_MAX))
        cuts.append(cut)
    return m, counts, cuts


def _chunk_reads(batches, m: int, max_read_len: Optional[int]):
    """(offsets, base bytes, max_read_len) of the first ``m`` records of every side.  ``max_read_len`` None: the longest
    read of the chunk, as the whole-file scans take the longest of the file."""
    offs = [b.offsets[:m + 1] for b in batches]
    # (at least one byte: a chunk whose records the filter or the duplicate removal all emptied still has an address)
    nb = [max(int(o[-1].item()), 1) for o in offs]
    mrl = max_read_len
    if mrl is None:
        mrl = max([int((o[1:] - o[:-1]).max().item()) for o in offs] + [1])
    return offs, nb, mrl


def _scan_step(indexer: Indexer, texts, batches, m: int, done: int, reads, prepared=None, check_lengths: bool = True):
    """How the first ``m`` records of every side (``reads``: what ``_chunk_reads`` gave) are scanned against one index:
    (``scan(**caps)`` -> ``PairScan``, the capacities with room for everything, ``gather(res, **cap)`` -> the
    ``HitNames`` of a scan's records, ``gather_records(res, **cap)`` -> their ``HitRecords``).  ``prepared``: the
    ``PreparedPairs`` of these pairs (multi_csv_scan.py), scanned in place of the records themselves."""
    from .fastq import fastq_cut_device
    from .hit_names import hit_names_device, hit_records_device
    from .single_end import scan_single_device
    single = len(texts) == 1
    offs, nb, mrl = reads
    if single:
        b = batches[0]

        def scan(**caps):
            return scan_single_device(indexer, b.bases[:nb[0]], b.quals[:nb[0]], offs[0], mrl, read_id_base=done,
                                      check_lengths=check_lengths, **caps)
        room = dict(hits_cap=m, bytes_cap=nb[0] + 64, retry_cap=m)
    else:
        room = dict(hits_cap=3 * m, bytes_cap=2 * sum(nb) + 64, retry_cap=3 * m)
        if prepared is not None:
            from .multi_csv_scan import scan_prepared_pairs_device

            def scan(**caps):
                return scan_prepared_pairs_device(indexer, prepared, pair_id_base=done, **caps)
        else:
            l, r = batches
            lean = l.qual_off is not None and r.qual_off is not None
            if not lean:   # one side has a quality line of another length than its sequence: both the full way
                l = l if l.qual_off is None else fastq_cut_device(indexer, texts[0])
                r = r if r.qual_off is None else fastq_cut_device(indexer, texts[1])
            lq, rq = (l.quals, r.quals) if lean else (l.quals[:nb[0]], r.quals[:nb[1]])
            qo = dict(l_qual_off=l.qual_off[:m], r_qual_off=r.qual_off[:m]) if lean else {}

            def scan(**caps):
                return scan_pairs_device(indexer, l.bases[:nb[0]], lq, offs[0], r.bases[:nb[1]], rq, offs[1], mrl,
                                         pair_id_base=done, **caps, **qo)

    sides = (texts[0], batches[0]) + (() if single else (texts[1], batches[1]))

    def gather(res, **cap):
        return hit_names_device(indexer, res, *sides, pair_id_base=done, **cap)

    def gather_records(res, **cap):
        return hit_records_device(indexer, res, *sides, pair_id_base=done, **cap)
    return scan, room, gather, gather_records


def fetch_records(recs, gather_records, res):
    """What a ``HitRecords`` downloads; records of more bytes than it had room for are gathered once more, with the
    room the first call asked for."""
    _, need, over, _ = (int(x) for x in recs.totals.cpu())
    if over:
        recs = gather_records(res, records_cap=need)
    return recs.download()


def _scan_alone(step, first_caps: dict, m: int, single: bool, names: bool, originals: bool = False):
    """One index's scan of a chunk with a read-back of its own (``scan_with_room``: ``first_caps``, then the room), the
    names of the hit records gathered behind the scan: (records, hit bases, hit qualities, names or None, totals); with
    ``originals`` their FASTQ records are gathered too, and follow as a sixth element."""
    scan, room, gather, gather_records = step
    # (the names are queued behind the scan: the record count stays on the device)
    behind = None
    if names or originals:
        def behind(res):
            return (gather(res) if names else None, gather_records(res) if originals else None)
    res, gathered, out = scan_with_room(scan, first_caps, room, behind)
    nm, recs = gathered or (None, None)
    name_list = None
    if names:
        _, need, over, _ = (int(x) for x in nm.totals.cpu())
        if over:   # names longer than 64 bytes on average: once more with the room the first call asked for
            nm = gather(res, names_cap=need)
        name_list = nm.download()
    out[3]["reads" if single else "pairs"] = m
    chunk = (out[0], out[1], out[2], name_list, out[3])
    return chunk + (fetch_records(recs, gather_records, res),) if originals else chunk


def _scan_records(indexer: Indexer, texts, batches, m: int, done: int, max_read_len: Optional[int], names: bool,
                  originals: bool = False):
    """The first ``m`` records of every side scanned — first with the library's default capacities — and the names of
    the hit records: (records, hit bases, hit qualities, names or None, totals), with ``originals`` the records' FASTQ
    records behind them."""
    step = _scan_step(indexer, texts, batches, m, done, _chunk_reads(batches, m, max_read_len))
    return _scan_alone(step, {}, m, len(texts) == 1, names, originals)


def _filter_chunk(indexer: Indexer, read_filter, batches, m: int):
    """The first ``m`` records of every side through the read filter (read_filter.py), queued behind the cut: (the
    batches it leaves, of ``m`` records each; its totals, on the device).  The records behind them are carried to the
    next chunk and filtered there."""
    from .read_filter import filter_reads_device
    *kept, totals = filter_reads_device(indexer, read_filter,
                                        *[b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in batches])
    return kept, totals


def _trim_chunk(indexer: Indexer, adapter_trim, batches, m: int):
    """The first ``m`` records of every side through the adapter trimming (adapter_trim.py), queued behind the cut and
    ahead of ``_filter_chunk``: (the batches it leaves, of ``m`` records each; its totals, on the device)."""
    from .adapter_trim import trim_adapters_device
    *kept, totals = trim_adapters_device(indexer, adapter_trim,
                                         *[b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in batches])
    return kept, totals


def _correct_chunk(indexer: Indexer, overlap_correct, batches, m: int):
    """The first ``m`` pairs through the overlap correction (overlap_correct.py), queued behind ``_umi_chunk`` and ahead
    of ``_trim_chunk``, which needs both mates uncut: (the batches it leaves, of ``m`` records each, corrected clones of
    the bases and qualities; its totals, on the device).  The pairs behind them are carried to the next chunk and
    corrected there, once."""
    from .overlap_correct import correct_overlaps_device
    *kept, totals = correct_overlaps_device(indexer, overlap_correct,
                                            *[b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in batches])
    return kept, totals


def _dedup_chunk(indexer: Indexer, dedup, batches, m: int, umi_codes=None):
    """The first ``m`` records of every side through the duplicate removal (dedup.py), queued behind ``_filter_chunk``:
    (the batches it leaves, of ``m`` records each; its totals, on the device).  Only these ``m`` are offered to the
    table: the records behind them are carried to the next chunk and offered there, once, so that the indices the table
    counts are the files'.  ``umi_codes``: what ``_umi_chunk`` gave for these ``m`` records, handed on only when set."""
    return dedup.apply(indexer, *[b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in batches],
                       **({} if umi_codes is None else {"umi_codes": umi_codes}))


def _umi_chunk(indexer: Indexer, umi, texts, batches, m: int):
    """The first ``m`` records of every side through the UMI step (umi.py), queued behind the cut and ahead of
    ``_trim_chunk``: (the batches it leaves; the ``m`` codes; its totals, on the device).  An inline source cuts the
    UMIs off — the batches then hold ``m`` records each; the name source reads the codes from the chunk's text (R1's)
    and leaves the batches as they are.  Only these ``m`` records are tagged: the ones behind them are carried to the
    next chunk and tagged there, once."""
    from .umi import cut_umis_device, name_umis_device
    if umi.inline:
        *kept, codes, totals = cut_umis_device(indexer, umi,
                                               *[b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in batches])
        return kept, codes, totals
    codes, totals = name_umis_device(indexer, texts[0], batches[0]._replace(n_records=m))
    return batches, codes, totals


def _measure_chunk(indexer: Indexer, qc, stage: str, batches, m: int) -> None:
    """The first ``m`` records of every side added to the tables of ``qc`` (read_qc.py) for ``stage``, queued behind
    what made them.  The records behind them are carried to the next chunk and measured there, once."""
    qc.measure(indexer, stage, *[b._replace(offsets=b.offsets[:m + 1], n_records=m) for b in batches])


def _scan_chunk(indexer: Indexer, side_names, texts, final, done: int, max_read_len: Optional[int], names: bool,
                scan_records=_scan_records, lean: Optional[bool] = None, *, read_filter=None, adapter_trim=None,
                qc=None, dedup=None, umi=None, write_reads=None, overlap_correct=None):
    """One chunk for ``ChunkStream.run``: the texts cut into records, the records all sides share scanned by
    ``scan_records``.  The result is (what the stream yields for the chunk or None, records scanned, whether the scan
    ends here).  ``lean``: whether the cut leaves the qualities in the text (default: pairs do).  ``read_filter``: a
    ``ReadFilter``, the records scanned go through the read filter between the cut — the full one, whatever ``lean``
    says — and the scan, and its totals are added to the totals of the chunk (of every index's, when ``scan_records``
    gives a list) under ``read_filter.COUNTER_KEYS``.  ``adapter_trim``: an ``AdapterTrim``, the same for the adapter
    trimming, which runs between the cut and the read filter; its totals go under
    ``adapter_trim.ADAPTER_COUNTER_KEYS``, in front of the read filter's.  ``qc``: a ``ReadQc``, the first ``m``
    records of every side — the rest are carried into the next chunk and measured there — are added to its tables
    between the cut, the full one again, and the trimming, and behind the last of the steps when any of them runs.
    ``dedup``: a ``Dedup``, the same for the duplicate removal, which runs last, behind the read filter — the full cut
    again; its totals go under ``dedup.DEDUP_COUNTER_KEYS``, behind the read filter's.  ``umi``: a ``Umi``, the UMI
    step (``_umi_chunk``) between ``qc``'s "before" stage and the trimming — an inline source needs the full cut, the
    name source alone does not; the codes it gives go to the duplicate removal, and its totals under
    ``umi.UMI_COUNTER_KEYS``, in front of the trimming's.  ``write_reads``: a ``ReadWriter`` with its files open, the
    first ``m`` records of every side as the last step leaves them are formatted as FASTQ text on the device
    (read_write.py) behind ``qc``'s "after" stage and ahead of the scan — the full cut again, for the names the chunk's
    texts and the cut's newline index, for ``umi_in_name`` the batches ahead of the UMI cut — and behind the chunk's
    read-back the text goes to the files' threads; its totals go under ``read_write.WRITE_COUNTER_KEYS``, behind the
    duplicate removal's.  The records carried over are written with the next chunk, once.  ``overlap_correct``: an
    ``OverlapCorrect``, the overlap correction (``_correct_chunk``) between the UMI step and the trimming — pairs only,
    the full cut again, and a step for ``qc``'s "after" stage; its totals go under
    ``overlap_correct.CORRECT_COUNTER_KEYS``, between the UMI step's and the trimming's."""
    from .fastq import fastq_cut_device
    umi_cuts = umi is not None and umi.inline
    if read_filter is not None or adapter_trim is not None or qc is not None or dedup is not None or umi_cuts:
        lean = False
    if write_reads is not None or overlap_correct is not None:
        lean = False
    # (pairs, lean: the qualities stay in the chunk's text, which lives in the slot's buffer until the scan below is
    #  done; single-end: gf_se_scan_device takes the qualities at the bases' offsets, so the full cut)
    lean = len(texts) > 1 if lean is None else lean
    batches = [fastq_cut_device(indexer, t, lean=lean) for t in texts]
    m, counts, cuts = _record_cuts(batches, texts, final, side_names)
    if qc is not None and m > 0:
        _measure_chunk(indexer, qc, "before", batches, m)
    if (read_filter is not None or adapter_trim is not None or dedup is not None or umi is not None
            or write_reads is not None or overlap_correct is not None) and m > 0:
        kept, counted = batches, {}
        if umi is not None:
            from .umi import umi_totals_counters
            kept, umi_codes, umi_totals = _umi_chunk(indexer, umi, texts, kept, m)
        if overlap_correct is not None:
            from .overlap_correct import correct_totals_counters
            kept, correct_totals = _correct_chunk(indexer, overlap_correct, kept, m)
        if adapter_trim is not None:
            from .adapter_trim import adapter_totals_counters
            kept, trim_totals = _trim_chunk(indexer, adapter_trim, kept, m)
        if read_filter is not None:
            from .read_filter import totals_counters
            kept, totals = _filter_chunk(indexer, read_filter, kept, m)
        if dedup is not None:
            from .dedup import dedup_totals_counters
            kept, dedup_totals = _dedup_chunk(indexer, dedup, kept, m,
                                              **({} if umi is None else {"umi_codes": umi_codes}))
        # (the name source moves no byte: alone it leaves nothing to measure "after", as on the whole-file routes)
        if qc is not None and (read_filter is not None or adapter_trim is not None or dedup is not None or umi_cuts
                               or overlap_correct is not None):
            _measure_chunk(indexer, qc, "after", kept, m)
        if write_reads is not None:
            formatted = write_reads.format_chunk(indexer, texts, batches, kept, m,
                                                 **({"pre": batches, "umi": umi} if write_reads.umi_in_name else {}))
        out = scan_records(indexer, texts, kept, m, done, max_read_len, names)
        if umi is not None:
            counted.update(umi_totals_counters(umi_totals.cpu().tolist()))
        if overlap_correct is not None:
            counted.update(correct_totals_counters(correct_totals.cpu().tolist()))
        if adapter_trim is not None:
            counted.update(adapter_totals_counters(trim_totals.cpu().tolist()))
        if read_filter is not None:
            counted.update(totals_counters(totals.cpu().tolist()))
        if dedup is not None:
            counted.update(dedup_totals_counters(dedup_totals.cpu().tolist(), dedup.remove))
        if write_reads is not None:   # (behind the chunk's read-back: the text is ready, and the copy waits for nothing)
            counted.update(write_reads.collect(formatted))
        for per_index in (out if isinstance(out, list) else [out]):
            per_index[4].update(counted)
    else:
        out = scan_records(indexer, texts, batches, m, done, max_read_len, names) if m > 0 else None
    # records pair up by position and the shorter file ends both (fastq_reader.rs:209-218): stop when a side that
    # has all its bytes has no record left
    last = any(f and c == m for f, c in zip(final, counts))
    # (starved: every complete record of the side was used, the other side is not behind it)
    return cuts, [c == m for c in counts], (out, m, last)


def _scan_source_stream(indexer: Indexer, sources, chunk_bytes: int, max_read_len: Optional[int], names: bool,
                        scan_records=_scan_records, lean: Optional[bool] = None, *, read_filter=None,
                        adapter_trim=None, qc=None, dedup=None, umi=None, write_reads=None, overlap_correct=None):
    """The chunk loop of both layouts: ``sources`` is (R1, R2) or (reads,).  Yields per chunk what ``scan_records`` gives
    for it — by default (records, hit bases, hit qualities, names or None, totals); ``multi_csv_scan`` plugs in the scan
    of one chunk against K indexes, with ``lean=False`` (``_scan_chunk``).  ``read_filter``: a ``ReadFilter``, handed
    to ``_scan_chunk`` (only when set); ``adapter_trim``: an ``AdapterTrim``, likewise; ``qc``: a ``ReadQc``, likewise;
    ``dedup``: a ``Dedup``, likewise; ``umi``: a ``Umi``, likewise.  ``write_reads``: a ``ReadWriter``, likewise; its
    files are opened before the first chunk, renamed to their names when the stream ends, and removed when it raises or
    is closed early.  ``overlap_correct``: an ``OverlapCorrect``, likewise."""
    import torch
    filtered = {} if read_filter is None else {"read_filter": read_filter}
    if overlap_correct is not None:
        filtered["overlap_correct"] = overlap_correct
    if adapter_trim is not None:
        filtered["adapter_trim"] = adapter_trim
    if qc is not None:
        filtered["qc"] = qc
    if dedup is not None:
        filtered["dedup"] = dedup
    if umi is not None:
        filtered["umi"] = umi
    if write_reads is not None:
        filtered["write_reads"] = write_reads
        write_reads.open(len(sources))
    h = indexer._handle()

    def copy(ptr: int, dst: int, n: int, stream: int) -> None:
        _lib.check(_lib.lib().gf_copy_from_host_device(h, ptr, dst, n, stream))
    try:
        stream = ChunkStream(sources, chunk_bytes, torch.device("cuda", indexer.info()["device"]), copy,
                             fill_read_sizes)
        side_names = [s.name for s in stream.sides]
        done = 0
        with closing(stream.run(lambda texts, final: _scan_chunk(indexer, side_names, texts, final, done, max_read_len,
                                                                 names, scan_records, lean, **filtered))) as chunks:
            for out, m, last in chunks:
                if out is not None:
                    yield out
                done += m
                if last:
                    break
    except BaseException:   # (a stream that is closed early too: half a file is no output)
        if write_reads is not None:
            write_reads.abort()
        raise
    if write_reads is not None:
        write_reads.finish()


def open_fastq_sources(opened, files, inflate: str = "host") -> list:
    """The byte sources of the FASTQ ``files``, entered into the ``ExitStack`` ``opened``: ``FastqReader.open_stream``,
    or with ``inflate`` "auto" / "device" a ``bgzf.BgzfSource`` for a BGZF file, whose compressed bytes are inflated on
    the device."""
    from .bgzf import open_source
    from .fastq import FastqReader
    sources = []
    for f in files:
        reader = FastqReader(f)
        sources.append(opened.enter_context(open_source(reader.m_filename, inflate, reader.open_stream)))
    return sources


def scan_pair_source_stream(indexer: Indexer, r1_source, r2_source, chunk_bytes: int = 128 << 20,
                            max_read_len: Optional[int] = 320, names: bool = True,
                            originals: bool = False, *, read_filter=None, adapter_trim=None,
                            qc=None, dedup=None, umi=None, write_reads=None,
                            overlap_correct=None) -> Iterator[Tuple[np.ndarray, bytes, bytes, Optional[List[bytes]], dict]]:
    """The paired-end scan of two byte sources of FASTQ text — anything with ``readinto(memoryview) -> int`` (0 at
    the end): ``ArraySource``, ``fastq.FastqReader.open_stream()``; or a ``bgzf.BgzfSource`` — chunk by chunk.  Yields,
    per chunk, (gf_pair_hit records with pair ids counted from the start of the files, the matched reads' bases, their qualities, the names of
    the records' reads (``hit_names_device``; None with ``names=False``), totals); ``totals["pairs"]`` is the chunk's
    pair count.  Records pair up by position; the shorter file ends both (fastq_reader.rs:209-218).  The next chunk of
    each source is read (gunzipped) and uploaded on host threads while the device works on the current one; the host
    holds two staging blocks of ``chunk_bytes`` per side.  ``max_read_len=None``: the longest read of each chunk.
    ``originals``: a sixth element per chunk, the FASTQ records of the hit records' pairs (``hit_records_device``: per
    record the (name, sequence, strand, quality) of R1 and of R2), gathered behind the scan before the chunk goes.
    ``read_filter``: a ``read_filter.ReadFilter``, every chunk's pairs go through the read filter between the cut —
    then the full one, the qualities at the bases' offsets — and the scan; the chunk's totals gain the filter's seven
    counts (``read_filter.COUNTER_KEYS``).  None (the default): nothing more is queued.  ``adapter_trim``: an
    ``adapter_trim.AdapterTrim``, every chunk's pairs go through the adapter trimming between the cut — the full one
    again — and the read filter or the scan; the chunk's totals gain its five counts
    (``adapter_trim.ADAPTER_COUNTER_KEYS``).  None (the default): nothing more is queued.  ``qc``: a
    ``read_qc.ReadQc``, every chunk's pairs are measured between the cut — the full one again — and the trimming, and
    behind the read filter when either of the two runs; what is yielded stays as it is.  None (the default): nothing
    more is queued.  ``dedup``: a ``dedup.Dedup``, every chunk's pairs go through the duplicate removal behind the read
    filter — the full cut again — and ``qc``'s "after" stage moves behind it; the chunk's totals gain its four counts
    (``dedup.DEDUP_COUNTER_KEYS``).  None (the default): nothing more is queued.  ``umi``: a ``umi.Umi``, every chunk's
    pairs go through the UMI step between ``qc``'s "before" stage and the trimming: an inline source cuts the UMIs off
    — the full cut again — the name source reads them from R1's names in the chunk's text; the codes go to ``dedup``,
    and the chunk's totals gain its five counts (``umi.UMI_COUNTER_KEYS``) in front of the trimming's.  A chunk tags
    the pairs it scans, never the ones it carries over.  None (the default): nothing more is queued.  ``write_reads``:
    a ``read_write.ReadWriter`` with ``out2``, every chunk's pairs that still have bases in both mates behind the last
    of these steps are formatted as FASTQ text on the device — the full cut again — and written to its two files by a
    thread each; the chunk's totals gain its three counts (``read_write.WRITE_COUNTER_KEYS``) behind the duplicate
    removal's.  A chunk writes the pairs it scans, never the ones it carries over; the files get their names when the
    stream ends and are removed when it raises.  Alone it rewrites the pairs whose mates both have bases.  None (the
    default): nothing more is queued.  ``overlap_correct``: an ``overlap_correct.OverlapCorrect``, every chunk's pairs go
    through the overlap correction between the UMI step and the trimming — the full cut again: inside the overlap of
    the mates a poor base that the mate's good base contradicts is rewritten from it, so that the trimming, the filter,
    the removal, ``qc``'s "after" stage, ``write_reads`` and the scan see corrected records; the chunk's totals gain its
    five counts (``overlap_correct.CORRECT_COUNTER_KEYS``) between the UMI step's and the trimming's.  A chunk corrects
    the pairs it scans, never the ones it carries over.  None (the default): nothing more is queued.  ``ValueError``
    for anything else."""
    from .dedup import need_dedup
    from .overlap_correct import need_overlap_correct
    from .read_qc import need_read_qc
    from .umi import need_umi
    need_overlap_correct(overlap_correct)
    if write_reads is not None:   # (checked first)
        from .read_write import need_read_writer
        need_read_writer(write_reads).need_route(("R1", "R2"), need_umi(umi))
    scan_records = partial(_scan_records, originals=True) if originals else _scan_records
    need_umi(umi)
    ahead = {k: v for k, v in (("read_filter", read_filter), ("adapter_trim", adapter_trim),
                               ("qc", need_read_qc(qc)), ("dedup", need_dedup(dedup)),
                               ("write_reads", write_reads), ("overlap_correct", overlap_correct)) if v is not None}
    if ahead or (umi is not None and umi.inline):
        return _scan_source_stream(indexer, (r1_source, r2_source), chunk_bytes, max_read_len, names, scan_records,
                                   lean=False, **ahead, **({} if umi is None else {"umi": umi}))
    return _scan_source_stream(indexer, (r1_source, r2_source), chunk_bytes, max_read_len, names, scan_records,
                               **({} if umi is None else {"umi": umi}))


def scan_pair_text_stream(indexer: Indexer, r1_text: np.ndarray, r2_text: np.ndarray, chunk_bytes: int = 128 << 20,
                          max_read_len: int = 320) -> Iterator[Tuple[np.ndarray, bytes, bytes, dict]]:
    """Yields, per chunk, what ``PairScan.download`` returns — (gf_pair_hit records with pair ids counted
    from the start of the files, the matched reads' bases, their qualities, totals) — for the FASTQ
    texts ``r1_text`` / ``r2_text`` (uint8 arrays; pinned memory makes the copies asynchronous).
    Records pair up by position; the shorter file ends both (fastq_reader.rs:209-218)."""
    for rec, hb, hq, _, tot in scan_pair_source_stream(indexer, ArraySource(r1_text), ArraySource(r2_text), chunk_bytes,
                                                       max_read_len, names=False):
        yield rec, hb, hq, tot


def scan_single_text_stream(indexer: Indexer, source, chunk_bytes: int = 128 << 20, max_read_len: Optional[int] = 320,
                            names: bool = True, originals: bool = False, *, read_filter=None, adapter_trim=None,
                            qc=None, dedup=None, umi=None, write_reads=None,
                            overlap_correct=None) -> Iterator[Tuple[np.ndarray, bytes, bytes, Optional[List[bytes]], dict]]:
    """The single-end counterpart: one byte source (a uint8 array is wrapped into an ``ArraySource``), scanned chunk by
    chunk with ``single_end.scan_single_device`` (``read_id_base`` = reads done so far).  Yields per chunk (records, hit
    bases, hit qualities, names, totals); ``totals["reads"]`` is the chunk's record count.  A final record without a
    trailing newline counts (fastq_reader.rs:75-147).  ``originals``: see ``scan_pair_source_stream``; one FASTQ record
    per hit record.  ``read_filter``, ``adapter_trim`` (which needs ``adapter_r1``), ``qc``, ``dedup``: see
    ``scan_pair_source_stream``.  ``umi``: likewise; "per_read" is "read1" here, and "read2" raises ``ValueError``.
    ``write_reads``: likewise, a ``ReadWriter`` without ``out2``: the reads that still have bases go to ``out1``.
    ``overlap_correct``: anything but None raises ``ValueError``, an ``OverlapCorrect`` too: the correction needs pairs."""
    from .dedup import need_dedup
    from .overlap_correct import need_pairs
    from .read_qc import need_read_qc
    from .umi import need_umi
    need_pairs(overlap_correct, False)
    if write_reads is not None:   # (checked first)
        from .read_write import need_read_writer
        need_read_writer(write_reads).need_route(("reads",), need_umi(umi))
    need_read_qc(qc)
    need_dedup(dedup)
    if need_umi(umi) is not None:
        umi.need_sides(1)
    if isinstance(source, np.ndarray):
        source = ArraySource(source)
    return _scan_source_stream(indexer, (source,), chunk_bytes, max_read_len, names,
                               partial(_scan_records, originals=True) if originals else _scan_records,
                               **({} if read_filter is None else {"read_filter": read_filter}),
                               **({} if adapter_trim is None else {"adapter_trim": adapter_trim}),
                               **({} if qc is None else {"qc": qc}),
                               **({} if dedup is None else {"dedup": dedup}),
                               **({} if umi is None else {"umi": umi}),
                               **({} if write_reads is None else {"write_reads": write_reads}))


def scan_pair_end_text(indexer: Indexer, r1_text: np.ndarray, r2_text: np.ndarray, chunk_bytes: int = 128 << 20,
                       threads: int = 8) -> Tuple[List[Tuple[int, ReadMatch]], dict]:
    """The whole paired-end scan of two FASTQ texts up to the ReadMatch list (before the filters):
    ([(pair index, ReadMatch)] in push order, counters)."""
    mapper = FusionMapper(indexer)
    found: List[Tuple[int, ReadMatch]] = []
    counters = {"pairs": 0, "merged_pairs": 0, "retried_reads": 0, "hits": 0, "chunks": 0}
    for rec, hb, hq, tot in scan_pair_text_stream(indexer, r1_text, r2_text, chunk_bytes):
        found += finish_pair_hits(mapper, rec, hb, hq, threads)
        for k in ("pairs", "merged_pairs", "retried_reads", "hits"):
            counters[k] += tot[k]
        counters["chunks"] += 1
    return found, counters
