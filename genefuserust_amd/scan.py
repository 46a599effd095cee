"""The front half of ``PairEndScanner::scan`` (src/core/pescanner.rs:78-518) from the reference's
own file formats: FASTA + fusion CSV -> index; R1/R2 FASTQ -> records -> per-pair policy
(merge, map, reverse-complement retries) -> ``ReadMatch`` lists, filtered and sorted the way
``FusionMapper::filter_matches`` (without ``remove_alignables``) and ``sort_matches`` do.

Glue only: every step is one of the mirrors in this package, and all compute goes through
libgfmatch.so.  ``scan_pair_end_report`` adds the back half (clustering, qualification, text and
JSON results: SURVEY.md §8(f)-4, ``fusion_result.py``).  ``remove_alignables`` (§8(f)-3, ``matcher.py``:
the reference's ``Matcher`` as it is — it removes nothing on a genome, and panics on small
references) is applied only on request.

Every file-level route (whole file, streamed, single-end on the device or the host, per CSV of multi-CSV mode) is
made of the same pieces, each written once here: ``open_index``; a producer of (matches found, counters before the
filter counts, counters after them) — ``pairs_found``, ``single_end_found``, ``streamed_found`` — that scans through
``read_pair.scan_with_room`` and names its matches by ``match_named``; ``finish_matches``; ``report_matches``.
"""
from __future__ import annotations

from contextlib import ExitStack, contextmanager
from typing import List, Tuple

from .fastq import FastqReader, FastqReaderPair, record_lines
from .fusion_mapper import FusionMapper, ReadMatch
from .fusion_result import FusionResult, Settings, cluster_matches, group_and_sort, report_json, report_text
from .indexer import FastaReader, Fusion, Indexer
from .read_pair import finish_pair_hits, scan_pairs_device, scan_with_room


def read_contigs(ref_file: str) -> dict:
    ref = FastaReader(ref_file, True)
    ref.read_all()
    return ref.m_all_contigs


class GeneSlices(list):
    """The gene slices of one fusion CSV, already cut out of the reference (``ref_cut.cut_gene_slices``): what
    ``open_index`` takes in place of the contigs."""


@contextmanager
def open_index(ref, fusion_csv: str, device: int = -1, ref_chunk_bytes: int = None, inflate: str = "host"):
    """FASTA (a file name, the contigs ``read_contigs`` gave, or the ``GeneSlices`` of this CSV) + fusion CSV -> (the
    open ``Indexer`` with its index made, the parsed fusions); the index is closed on the way out.

    ``ref_chunk_bytes`` (with a file name): None reads the FASTA whole on the host (``read_contigs``).  With a value
    the file is streamed in chunks of that many bytes of plain text and the gene slices are cut out on the device
    (``ref_cut.cut_gene_slices``): the same index, and no contigs on the host (``Indexer.m_reference`` is None).

    ``inflate`` (with ``ref_chunk_bytes``; ``ValueError`` without): "host" gunzips a ``.gz`` file on the host as it is
    read; "auto" sends a BGZF file's compressed bytes to the device and inflates them there (bgzf.py), any other file
    as "host" does; "device" does so too and raises ``ValueError`` for a ``.gz`` file that is not BGZF."""
    from .bgzf import need_chunks
    need_chunks(inflate, ref_chunk_bytes is not None, "ref_chunk_bytes")
    fusions = Fusion.parse_csv(fusion_csv)
    if isinstance(ref, str) and ref_chunk_bytes is not None:
        from .ref_cut import cut_gene_slices
        ref = GeneSlices(cut_gene_slices(ref, [fusions], ref_chunk_bytes, device, inflate)[0])
    if isinstance(ref, GeneSlices):
        ix = Indexer(None, fusions, device, gene_slices=ref)
    else:
        ix = Indexer(read_contigs(ref) if isinstance(ref, str) else ref, fusions, device)
    ix.make_index()
    try:
        yield ix, fusions
    finally:
        ix.close()


def match_named(m: ReadMatch, name_of_side) -> ReadMatch:
    """``m`` with the name a match carries: R2's for a match on R2 (or its reverse complement), anything else R1's
    (``name_of_side("r2")`` / ``name_of_side("r1")``); a merged read adds the suffix of read.rs:372."""
    m.m_name = name_of_side("r2" if m.m_source == "r2" else "r1")
    if m.m_source == "merged":
        m.m_name += b" merged_diff_%d" % m.m_merge_diff
    return m


def named_from_records(hits, l, ltext: bytes, r=None, rtext: bytes = None, originals: bool = False) -> List[ReadMatch]:
    """The matches of ``hits`` ((record index, match) pairs) named from the host texts of a whole-file cut.
    ``originals``: each also gets its ``m_original_reads``, the FASTQ record of R1 and, for pairs, of R2 — both,
    whichever read matched (``add_original_pair``, pescanner.rs:456-511; ``add_original_read``, sescanner.rs:191-197)."""
    sides = {"r1": (l, ltext), "r2": (r, rtext)}
    if originals:
        for i, m in hits:
            m.m_original_reads = [record_lines(*sides[side], i) for side in (("r1",) if r is None else ("r1", "r2"))]
    return [match_named(m, lambda side: record_lines(*sides[side], i)[0]) for i, m in hits]


def named_from_device(hits, rec, names, originals=None) -> List[ReadMatch]:
    """The matches of a streamed chunk named from the names gathered on the device, one per ``gf_pair_hit`` record.
    ``originals``: what ``HitRecords.download`` gave for the same records, each match's ``m_original_reads``."""
    side_of = ("r1", "r1", "r2")   # by the record's source: merged, r1, r2
    name_of = {(int(h["pair_id"]), side_of[int(h["source"])]): nm for h, nm in zip(rec, names)}
    if originals is not None:
        records_of = {int(h["pair_id"]): o for h, o in zip(rec, originals)}   # (the same for every record of a pair)
        for i, m in hits:
            m.m_original_reads = list(records_of[i])
    return [match_named(m, lambda side: name_of[(i, side)]) for i, m in hits]


def route_counters(count_key: str, n: int, n_found: int, tot: dict = None, chunks: int = None) -> Tuple[dict, dict]:
    """A route's counters, as (those in front of the filter counts, those behind them): ``count_key`` is "pairs" or
    "reads", ``tot`` the totals of the device scan (None: the host route), ``chunks`` set by the streamed routes."""
    before, after = {count_key: n, "matches_before_filtering": n_found}, {}
    if count_key == "pairs":
        before.update(merged_pairs=tot["merged_pairs"], retried_reads=tot["retried_reads"])
    elif tot is not None:
        after["retried_reads"] = tot["retried_reads"]
    if chunks is not None:
        after["chunks"] = chunks
    return before, after


def filtered_reads(ix: Indexer, read_filter, *batches):
    """The ``FastqBatch``es (a file's records, or a pair's) through the read filter on the index's device
    (read_filter.py): (the batches it leaves, ``counted(produced)``).  ``counted`` adds the filter's seven totals to
    the end of a producer's counters in front of the filter counts.  ``read_filter`` None: the batches as they are,
    nothing queued, and ``counted`` changes nothing."""
    if read_filter is None:
        return batches, lambda produced: produced
    from .read_filter import filter_reads_device, totals_counters
    *kept, totals = filter_reads_device(ix, read_filter, *batches)

    def counted(produced):
        found, before, after = produced
        return found, {**before, **totals_counters(totals.cpu().tolist())}, after
    return tuple(kept), counted


def tagged_reads(ix: Indexer, umi, text: bytes, *batches):
    """The ``FastqBatch``es (a file's records, or a pair's) through the UMI step on the index's device (umi.py), ahead
    of ``trimmed_reads``: (the batches it leaves, the records' UMI codes or None, ``counted(produced)``).  An inline
    source cuts the UMIs off the records; the name source reads them from ``text``, the host text of the file (of R1),
    which goes to the device once more for it, and leaves the batches as they are.  ``counted`` adds the five ``umi_*``
    totals to the end of a producer's counters in front of the filter counts — so it is applied first — and ``umi``
    None gives the batches as they are, no codes, nothing queued, and a ``counted`` that changes nothing."""
    if umi is None:
        return batches, None, lambda produced: produced
    from .umi import cut_umis_device, name_umis_device, umi_totals_counters
    umi.need_sides(len(batches))
    if umi.inline:
        *kept, codes, totals = cut_umis_device(ix, umi, *batches)
    else:
        import warnings
        import torch
        with warnings.catch_warnings():
            # (the upload only reads the host text: no copy of it into a writable buffer first)
            warnings.simplefilter("ignore", UserWarning)
            d_text = torch.frombuffer(text, dtype=torch.uint8).to(batches[0].bases.device) if text \
                else torch.empty(0, dtype=torch.uint8, device=batches[0].bases.device)
        kept, (codes, totals) = batches, name_umis_device(ix, d_text, batches[0])

    def counted(produced):
        found, before, after = produced
        return found, {**before, **umi_totals_counters(totals.cpu().tolist())}, after
    return tuple(kept), codes, counted


def deduplicated_reads(ix: Indexer, dedup, *batches, umi_codes=None):
    """The ``FastqBatch``es (a file's records, or a pair's) through the duplicate removal on the index's device
    (dedup.py), behind ``filtered_reads`` and in front of the scan: (the batches it leaves, ``counted(produced)``).
    ``counted`` adds the four ``dedup_*`` totals to the end of a producer's counters in front of the filter counts — so it
    is applied behind ``filtered_reads``' — and ``dedup`` None gives the batches as they are, nothing queued, and a
    ``counted`` that changes nothing.  ``umi_codes``: what ``tagged_reads`` gave, handed to ``Dedup.apply`` only when
    set."""
    if dedup is None:
        return batches, lambda produced: produced
    from .dedup import dedup_totals_counters
    kept, totals = dedup.apply(ix, *batches, **({} if umi_codes is None else {"umi_codes": umi_codes}))

    def counted(produced):
        found, before, after = produced
        return found, {**before, **dedup_totals_counters(totals.cpu().tolist(), dedup.remove)}, after
    return tuple(kept), counted


def trimmed_reads(ix: Indexer, adapter_trim, *batches):
    """The ``FastqBatch``es (a file's records, or a pair's) through the adapter trimming on the index's device
    (adapter_trim.py), ahead of ``filtered_reads``: (the batches it leaves, ``counted(produced)``).  ``counted`` adds the
    trimming's five totals to the end of a producer's counters in front of the filter counts — so it is applied before
    ``filtered_reads``' — and ``adapter_trim`` None gives the batches as they are, nothing queued, and a ``counted``
    that changes nothing."""
    if adapter_trim is None:
        return batches, lambda produced: produced
    from .adapter_trim import adapter_totals_counters, trim_adapters_device
    *kept, totals = trim_adapters_device(ix, adapter_trim, *batches)

    def counted(produced):
        found, before, after = produced
        return found, {**before, **adapter_totals_counters(totals.cpu().tolist())}, after
    return tuple(kept), counted


def corrected_reads(ix: Indexer, overlap_correct, *batches):
    """The ``FastqBatch``es of a pair through the overlap correction on the index's device (overlap_correct.py), behind
    ``tagged_reads`` and ahead of ``trimmed_reads``, which needs both mates uncut: (the batches it leaves,
    ``counted(produced)``).  ``counted`` adds the correction's five totals to the end of a producer's counters in front
    of the filter counts — so it is applied before ``trimmed_reads``' — and ``overlap_correct`` None gives the batches
    as they are, nothing queued, and a ``counted`` that changes nothing."""
    if overlap_correct is None:
        return batches, lambda produced: produced
    from .overlap_correct import correct_overlaps_device, correct_totals_counters
    *kept, totals = correct_overlaps_device(ix, overlap_correct, *batches)

    def counted(produced):
        found, before, after = produced
        return found, {**before, **correct_totals_counters(totals.cpu().tolist())}, after
    return tuple(kept), counted


def measured_reads(ix: Indexer, qc, stage: str, *batches) -> None:
    """The ``FastqBatch``es added to the tables of ``qc`` (a ``read_qc.ReadQc``) for ``stage``, "before" or "after",
    on the index's device; at "before" the insert lengths of a pair too.  ``qc`` None: nothing is queued."""
    if qc is not None:
        qc.measure(ix, stage, *batches)


def finish_matches(found: List[ReadMatch], mapper, deletion_threshold: int, remove_alignables: bool, before: dict,
                   after: dict, tail: str = "host", *, alignable_filter: str = None) -> Tuple[List[ReadMatch], dict]:
    """The tail of every route: the filters, (matches kept in ``sort_matches`` order, counters).  ``tail``: "host", a
    library call per match and per comparison; "device", the reasons of all matches in one call on the index's device
    and the order through ``numpy.lexsort`` (report_tail.py) — the same matches and counters.  ``alignable_filter``:
    None, or "genome": the reads of the matches that the other filters keep are tested against the whole reference in
    one call on the index's device (alignable.py), the alignable ones dropped and counted as ``genome_alignables``
    behind the filter counts; ``ValueError`` for anything else, and together with ``remove_alignables``."""
    from . import alignable, report_tail
    genome = alignable.need_filter(alignable_filter, remove_alignables)
    if report_tail.need_tail(tail):
        kept, removed = report_tail.filter_matches_device(found, deletion_threshold, mapper.m_indexer.info()["device"])
    else:
        kept, removed = mapper.filter_matches(found, deletion_threshold)
    if remove_alignables:  # (the reference always does: a whole-genome scan that removes nothing)
        kept, removed["alignables"] = mapper.remove_alignables(kept)
    if genome:
        kept, removed["genome_alignables"] = alignable.remove_genome_alignables(
            kept, mapper.m_indexer.get_ref(), mapper.m_indexer.info()["device"])
    sort = report_tail.order_matches if tail == "device" else mapper.sort_matches
    return sort(kept), {**before, **removed, **after}


def report_matches(kept: List[ReadMatch], counters: dict, fusions, fusion_seq, settings: Settings,
                   tail: str = "host", device: int = -1) -> Tuple[List[FusionResult], dict]:
    """Per-gene-pair sort -> cluster -> qualified fusions, most supported first; the counters add ``fusions``.
    ``tail``: "host", ``fusion_result.cluster_matches``; "device", ``report_tail.cluster_matches_device`` on
    ``device`` — the same results."""
    from . import report_tail
    if report_tail.need_tail(tail):
        results = report_tail.cluster_matches_device(group_and_sort(kept, len(fusions), report_tail.order_matches),
                                                     fusions, fusion_seq, settings, device)
    else:
        results = cluster_matches(group_and_sort(kept, len(fusions)), fusions, fusion_seq, settings)
    counters["fusions"] = len(results)
    return results, counters


def pairs_found(mapper: FusionMapper, reads, max_len: int, scan,
                originals: bool = False) -> Tuple[List[ReadMatch], dict, dict]:
    """The matches of the pairs ``reads`` (``FastqReaderPair.read_all_device``) in push order, and their counters:
    ``scan(**caps)`` is the device scan of those pairs (a ``PairScan``)."""
    (l, ltext), (r, rtext) = reads
    n = l.n_records
    first = max(1024, n // 8)
    rec, hb, hq, tot = scan_with_room(
        scan, dict(hits_cap=first, bytes_cap=first * 2 * max_len),
        dict(hits_cap=3 * n, bytes_cap=2 * int(l.bases.numel() + r.bases.numel()) + 64, retry_cap=3 * n))[2]
    found = named_from_records(finish_pair_hits(mapper, rec, hb, hq), l, ltext, r, rtext, originals)
    return (found, *route_counters("pairs", n, len(found), tot))


def single_end_found(ix: Indexer, mapper: FusionMapper, b, text: bytes,
                     originals: bool = False) -> Tuple[List[ReadMatch], dict, dict]:
    """The matches of a FASTQ batch in HBM, in read order, through one device call, and their counters."""
    from .single_end import scan_single_device
    n = b.n_records
    max_len = max(b.max_read_len(), 1)
    first = max(1024, n // 8)
    rec, hb, hq, tot = scan_with_room(
        lambda **caps: scan_single_device(ix, b.bases, b.quals, b.offsets, max_len, **caps),
        dict(hits_cap=first, bytes_cap=first * max_len),
        dict(hits_cap=max(n, 1), bytes_cap=int(b.bases.numel()) + 64, retry_cap=max(n, 1)))[2]
    found = named_from_records(finish_pair_hits(mapper, rec, hb, hq), b, text, originals=originals)
    return (found, *route_counters("reads", n, len(found), tot))


def _single_end_host_found(mapper: FusionMapper, b, text: bytes,
                           originals: bool = False) -> Tuple[List[ReadMatch], dict, dict]:
    """The same matches with the records on the host: ``FusionMapper.scan_single_end``, the tail per matched read."""
    off = b.offsets.cpu().numpy()
    bases, quals = b.bases.cpu().numpy().tobytes(), b.quals.cpu().numpy().tobytes()
    hits = []
    for i, m in enumerate(mapper.scan_single_end([bases[off[i]:off[i + 1]] for i in range(b.n_records)])):
        if m is None:
            continue
        q = quals[off[i]:off[i + 1]]
        m.m_quality = q[::-1] if m.m_reversed else q
        m.m_source = "r1"
        hits.append((i, m))
    found = named_from_records(hits, b, text, originals=originals)
    return (found, *route_counters("reads", b.n_records, len(found)))


def streamed_found(ix: Indexer, mapper: FusionMapper, files, chunk_bytes: int, inflate: str = "host",
                   originals: bool = False, *, read_filter=None,
                   adapter_trim=None, qc=None, dedup=None, umi=None,
                   write_reads=None, overlap_correct=None) -> Tuple[List[ReadMatch], dict, dict]:
    """The matches of the FASTQ files ``files`` ((R1, R2) or (reads,)) streamed in chunks (scan_stream.py), in push
    order, each named from its chunk's device-gathered names, and their counters.  ``inflate``: see ``open_index``.
    ``originals``: the matches' FASTQ records are gathered on the device too (``hit_names.hit_records_device``).
    ``read_filter``: a ``ReadFilter``, every chunk's records go through the read filter ahead of the scan
    (``scan_stream._scan_chunk``) and its totals, summed over the chunks, end the counters in front of the filter
    counts.  ``adapter_trim``: an ``AdapterTrim``, every chunk's records go through the adapter trimming ahead of that,
    and its five totals stand in front of the read filter's.  ``qc``: a ``ReadQc``, every chunk's records are measured
    before and behind the two (``scan_stream._scan_chunk``); the counters stay as they are.  ``dedup``: a ``Dedup``,
    every chunk's records go through the duplicate removal behind the read filter, and its four totals stand behind
    the read filter's.  ``umi``: a ``Umi``, every chunk's records go through the UMI step ahead of the adapter
    trimming, and its five totals stand in front of the trimming's.  ``write_reads``: a ``ReadWriter``, every chunk's
    records that are left with bases are written to its files, and its three totals stand behind the duplicate
    removal's.  ``overlap_correct``: an ``OverlapCorrect``, every chunk's pairs go through the overlap correction
    between the UMI step and the trimming, and its five totals stand between theirs."""
    from .adapter_trim import ADAPTER_COUNTER_KEYS
    from .overlap_correct import CORRECT_COUNTER_KEYS
    from .dedup import DEDUP_COUNTER_KEYS
    from .read_filter import COUNTER_KEYS
    from .scan_stream import open_fastq_sources, scan_pair_source_stream, scan_single_text_stream
    from .umi import UMI_COUNTER_KEYS
    count_key = "pairs" if len(files) == 2 else "reads"
    stream = scan_pair_source_stream if len(files) == 2 else scan_single_text_stream
    found: List[ReadMatch] = []
    sums = {count_key: 0, "merged_pairs": 0, "retried_reads": 0}
    extra = (() if umi is None else UMI_COUNTER_KEYS) + (() if overlap_correct is None else CORRECT_COUNTER_KEYS) \
        + (() if adapter_trim is None else ADAPTER_COUNTER_KEYS) \
        + (() if read_filter is None else COUNTER_KEYS) + (() if dedup is None else DEDUP_COUNTER_KEYS)
    if write_reads is not None:
        from .read_write import WRITE_COUNTER_KEYS
        extra += WRITE_COUNTER_KEYS
    sums.update(dict.fromkeys(extra, 0))
    chunks = 0
    with ExitStack() as opened:
        sources = open_fastq_sources(opened, files, inflate)
        # (originals=False, read_filter=None, adapter_trim=None, qc=None, dedup=None, umi=None, write_reads=None and
        #  overlap_correct=None are not passed on: the stream is then called as it always was)
        for rec, hb, hq, names, tot, *orig in stream(ix, *sources, chunk_bytes, max_read_len=None,
                                                     **({"originals": True} if originals else {}),
                                                     **({"read_filter": read_filter} if read_filter is not None else {}),
                                                     **({"adapter_trim": adapter_trim} if adapter_trim is not None else {}),
                                                     **({"qc": qc} if qc is not None else {}),
                                                     **({"dedup": dedup} if dedup is not None else {}),
                                                     **({"umi": umi} if umi is not None else {}),
                                                     **({"write_reads": write_reads} if write_reads is not None
                                                        else {}),
                                                     **({"overlap_correct": overlap_correct} if overlap_correct is not None else {})):
            found += named_from_device(finish_pair_hits(mapper, rec, hb, hq), rec, names, *orig)
            for k in sums:
                sums[k] += tot[k]
            chunks += 1
    before, after = route_counters(count_key, sums[count_key], len(found), sums, chunks)
    before.update({k: sums[k] for k in extra})
    return found, before, after


def _route_inflate(inflate, chunk_bytes, ref_chunk_bytes):
    """(``inflate`` for the FASTQ files, for the reference): it applies where a file is streamed, and raises
    ``ValueError`` where none is."""
    from .bgzf import need_chunks
    need_chunks(inflate, chunk_bytes is not None or ref_chunk_bytes is not None, "chunk_bytes or ref_chunk_bytes")
    return (inflate if chunk_bytes is not None else "host"), (inflate if ref_chunk_bytes is not None else "host")


def _cuts(umi) -> bool:
    """Whether the UMI step changes the records: an inline source does, the name source and None do not."""
    return umi is not None and umi.inline


def _need_whole_contigs(alignable_filter, remove_alignables, ref_chunk_bytes) -> None:
    """``ValueError`` for an ``alignable_filter`` that ``finish_matches`` refuses, and for the genome filter with a
    streamed reference: before any file is opened."""
    from .alignable import need_filter
    if need_filter(alignable_filter, remove_alignables) and ref_chunk_bytes is not None:
        raise ValueError("alignable_filter=%r needs whole contigs; ref_chunk_bytes cuts only the gene slices out of the "
                         "reference" % (alignable_filter,))


def _pair_end_matches(ref_file, fusion_csv, read1_file, read2_file, device, deletion_threshold, remove_alignables,
                      chunk_bytes, ref_chunk_bytes=None, inflate="host", tail="host", originals=False,
                      alignable_filter=None, read_filter=None, adapter_trim=None, *, qc=None, dedup=None, umi=None,
                      write_reads=None, overlap_correct=None):
    """(matches kept, counters, fusions, fusion sequences): ``scan_pair_end_files`` and what the report needs."""
    if write_reads is not None:   # (checked first)
        from .read_write import need_read_writer
        need_read_writer(write_reads)
    from .adapter_trim import need_adapter_trim
    from .dedup import need_dedup
    from .read_filter import need_read_filter
    from .read_qc import need_read_qc
    from .report_tail import need_tail
    from .umi import need_umi
    need_tail(tail)
    need_read_filter(read_filter)
    need_adapter_trim(adapter_trim)
    need_read_qc(qc)
    need_dedup(dedup)
    need_umi(umi)
    from .overlap_correct import need_overlap_correct
    need_overlap_correct(overlap_correct)
    if write_reads is not None:
        write_reads.need_route((read1_file, read2_file), umi, chunk_bytes is not None)
    _need_whole_contigs(alignable_filter, remove_alignables, ref_chunk_bytes)
    if remove_alignables and ref_chunk_bytes is not None:
        raise ValueError("remove_alignables needs whole contigs; ref_chunk_bytes cuts only the gene slices out of the "
                         "reference")
    fq_inflate, ref_inflate = _route_inflate(inflate, chunk_bytes, ref_chunk_bytes)
    with open_index(ref_file, fusion_csv, device, ref_chunk_bytes, ref_inflate) as (ix, fusions):
        mapper = FusionMapper(ix)
        if chunk_bytes is not None:
            produced = streamed_found(ix, mapper, (read1_file, read2_file), chunk_bytes, fq_inflate, originals,
                                      **({"read_filter": read_filter} if read_filter is not None else {}),
                                      **({"adapter_trim": adapter_trim} if adapter_trim is not None else {}),
                                      **({"qc": qc} if qc is not None else {}),
                                      **({"dedup": dedup} if dedup is not None else {}),
                                      **({"umi": umi} if umi is not None else {}),
                                      **({"write_reads": write_reads} if write_reads is not None else {}),
                                      **({"overlap_correct": overlap_correct} if overlap_correct is not None else {}))
        else:
            (l, ltext), (r, rtext) = FastqReaderPair.from_paths(read1_file, read2_file).read_all_device(ix)
            measured_reads(ix, qc, "before", l, r)
            (l, r), codes, tagged = tagged_reads(ix, umi, ltext, l, r)
            corrected = None   # (the helper is called only when the step is asked for)
            if overlap_correct is not None:
                (l, r), corrected = corrected_reads(ix, overlap_correct, l, r)
            (l, r), trimmed = trimmed_reads(ix, adapter_trim, l, r)
            (l, r), counted = filtered_reads(ix, read_filter, l, r)
            (l, r), deduplicated = deduplicated_reads(ix, dedup, l, r, **({} if codes is None else {"umi_codes": codes}))
            if (adapter_trim is not None or read_filter is not None or dedup is not None or _cuts(umi)
                    or overlap_correct is not None):
                measured_reads(ix, qc, "after", l, r)
            reads = (l, ltext), (r, rtext)
            max_len = max(l.max_read_len(), r.max_read_len(), 1)
            # the records never leave HBM between the FASTQ cut and the hit list: one device call for the pack
            produced = tagged(pairs_found(
                mapper, reads, max_len, lambda **caps: scan_pairs_device(
                    ix, l.bases, l.quals, l.offsets, r.bases, r.quals, r.offsets, max_len, **caps), originals))
            if corrected is not None:
                produced = corrected(produced)
            produced = deduplicated(counted(trimmed(produced)))
        kept, counters = finish_matches(produced[0], mapper, deletion_threshold, remove_alignables, *produced[1:],
                                        tail=tail, alignable_filter=alignable_filter)
        return kept, counters, fusions, list(ix.m_fusion_seq)


def scan_pair_end_files(ref_file: str, fusion_csv: str, read1_file: str, read2_file: str, device: int = -1,
                        deletion_threshold: int = 50, remove_alignables: bool = False,
                        chunk_bytes: int = None, ref_chunk_bytes: int = None,
                        inflate: str = "host", tail: str = "host",
                        originals: bool = False, *, alignable_filter: str = None,
                        read_filter=None, adapter_trim=None, qc=None,
                        dedup=None, umi=None, write_reads=None,
                        overlap_correct=None) -> Tuple[List[ReadMatch], dict]:
    """Returns (matches kept, in ``sort_matches`` order; counters).  Each match carries the name
    of the read it was found on (``match_named``).

    ``chunk_bytes``: None reads both files whole.  With a value they are streamed in chunks of that many bytes of
    plain text (scan_stream.scan_pair_source_stream: read, gunzipped and uploaded while the previous chunk is
    scanned, the names of the matched reads gathered on the device), so that neither the host nor the device ever
    holds a file; the matches and counters are the same, and the counters add ``chunks``.

    ``ref_chunk_bytes``: None reads the reference FASTA whole on the host.  With a value it is streamed in chunks too
    and the gene slices are cut out on the device (``open_index``); matches and counters are the same.
    ``remove_alignables`` needs whole contigs and raises ``ValueError`` with it.

    ``inflate``: where ``.gz`` files that are streamed are inflated — the FASTQ files with ``chunk_bytes``, the
    reference with ``ref_chunk_bytes``; ``ValueError`` for anything but "host" with neither.  "host" (the default):
    gunzipped on the host as they are read.  "auto": a file whose first member is BGZF (bgzip's and the sequencers'
    format) goes to the device compressed and is inflated there (bgzf.py); any other file as "host" does.  "device":
    as "auto", but a ``.gz`` file that is not BGZF raises ``ValueError``.  Matches and counters are the same; a member
    that fails raises ``gzip.BadGzipFile``, a file that ends inside a member ``EOFError``, a member that is not BGZF
    behind the first ``ValueError``.

    ``tail``: where the filters and the sort behind every route run — "host" (the default), a library call per match
    and per comparison; "device", all matches at once (report_tail.py: ``gf_rp_filter_device`` on the index's device,
    the order through ``numpy.lexsort``).  Matches and counters are the same; anything else raises ``ValueError``.

    ``originals``: every match also carries ``m_original_reads``, the FASTQ records of both mates of its pair as
    (name, sequence, strand, quality) — what the HTML report shows under a supporting read.  The whole-file route cuts
    them from the host text; the streamed route gathers them on the device behind each chunk's scan
    (``hit_names.hit_records_device``).  The same on every route; without it nothing more is queued or allocated.

    ``alignable_filter``: None (the default), or "genome": a last filter that works, on the device (alignable.py) — a
    match whose read lies end to end somewhere in the reference (either strand, fewer than 10 bases outside exact
    16-base windows, no indels) is dropped and counted as ``genome_alignables``.  It needs whole contigs: ``ValueError``
    with ``ref_chunk_bytes``, with ``remove_alignables`` (the reference's own filter as it is), and for any other
    value.

    ``read_filter``: None (the default), or a ``read_filter.ReadFilter``: the records go through a quality filter on
    the device between the FASTQ cut and the scan (read_filter.py) — poly-G and low-quality tails are cut off, and a
    pair with a mate that is then too short, holds too many N or too many low bases is scanned as two empty reads.
    The record indices stay, so names and ``m_original_reads`` are those of the records as the sequencer wrote them.
    The counters gain ``reads_passed``, ``reads_trimmed``, ``bases_trimmed``, ``reads_too_short``,
    ``reads_too_many_n``, ``reads_low_quality`` and ``reads_mate_failed`` in front of the filter counts, the same on
    every route; ``pairs`` keeps counting every record.  ``ValueError`` for anything else.  Without it nothing more is
    queued or allocated.

    ``adapter_trim``: None (the default), or an ``adapter_trim.AdapterTrim``: the records are cut to the insert on the
    device between the FASTQ cut and the read filter (adapter_trim.py) — a pair whose mates read through a short
    fragment into the adapters by the largest insert length at which they are each other's reverse complement, after
    which ``fast_merge`` merges them; a read without such a mate by its adapter's sequence.  The record indices stay,
    so names and ``m_original_reads`` are those of the records as the sequencer wrote them.  The counters gain
    ``adapter_reads_cut``, ``adapter_bases_cut``, ``adapter_cut_by_overlap``, ``adapter_cut_by_sequence`` and
    ``adapter_overlapping_pairs`` in front of the read filter's keys, the same on every route.  ``ValueError`` for
    anything else.  Without it nothing more is queued or allocated.

    ``qc``: None (the default), or a ``read_qc.ReadQc``: the records are measured on the device (read_qc.py) between
    the FASTQ cut and the adapter trimming — per-cycle quality and base content, read lengths, and the pairs' insert
    sizes — and again behind the read filter when either of the two runs; ``qc.result()`` has the tables and
    ``read_qc.report_json`` the document.  Matches and counters are those of the scan without it, on every route.
    ``ValueError`` for anything else.  Without it nothing more is queued or allocated.

    ``dedup``: None (the default), or a ``dedup.Dedup``: duplicate pairs are found on the device (dedup.py) behind the
    read filter — so by the bases of the trimmed records — and in front of the scan: of the pairs with the same bases,
    case folded, the first in file order is scanned and every other one as two empty reads (``Dedup(remove=False)`` only
    counts them).  The record indices stay, so a match is named after the first copy.  ``qc``'s "after" stage is then
    measured behind this step.  The counters gain ``dedup_checked``, ``dedup_unique``, ``dedup_duplicates`` and
    ``dedup_bases_removed`` behind the read filter's keys, the same on every route; ``dedup.result()`` has the rate and
    the histogram.  One ``Dedup`` handed to two scans removes the duplicates across them.  ``ValueError`` for anything
    else.  Without it nothing more is queued or allocated.

    ``umi``: None (the default), or a ``umi.Umi``: the library's unique molecular identifiers (umi.py), handled on the
    device between ``qc``'s "before" stage and the adapter trimming.  An inline source ("read1", "read2", "per_read")
    takes the first ``length`` bases and ``skip`` bases of spacer off the mates it names, so that they are neither
    merged, nor mapped, nor hashed as genome; a pair with a mate shorter than that is scanned as two empty reads.  The
    name source reads the UMI behind the last ':' of the first token of R1's name and moves no byte.  With ``dedup``
    every record's UMI code is mixed into its key: two pairs are duplicates when their bases and their UMIs are equal, a
    pair without a UMI by its bases alone.  Without ``dedup`` the inline sources still cut, the name source only counts.
    The record indices stay, so names and ``m_original_reads`` are those of the sequencer.  The counters gain
    ``umi_reads_tagged``, ``umi_missing``, ``umi_with_n``, ``umi_bases_cut`` and ``umi_too_short`` in front of the
    adapter trimming's keys, the same on every route.  ``ValueError`` for anything else.  Without it nothing more is
    queued or allocated.

    ``write_reads``: None (the default), or a ``read_write.ReadWriter``: the pairs whose mates both still have bases
    behind the last of these steps are written out as FASTQ files (read_write.py), in file order, R1's to ``out1`` and
    R2's to ``out2`` — the name lines as the sequencer wrote them, the bases and qualities as the steps left them, and
    with ``umi_in_name`` the inline UMI that ``umi`` cut off as ``:UMI`` at the end of the name's first token.  The text
    is formatted on the device per chunk, behind ``qc``'s "after" stage and ahead of the scan, and written by a thread
    per file; a name that ends in ``.gz`` is compressed by the host's zlib.  Streamed routes only: ``ValueError`` without
    ``chunk_bytes``, for an output that is an input, and for ``umi_in_name`` without an inline ``umi``.  Alone it
    rewrites the pairs whose mates both have bases.  The counters gain ``written_records``, ``written_bases`` and
    ``written_bytes`` behind the duplicate removal's keys; matches and the other counters are those of the scan
    without it.  Without it nothing more is queued or allocated.

    ``overlap_correct``: None (the default), or an ``overlap_correct.OverlapCorrect``: bases inside the overlap of a
    pair are corrected from the mate on the device (overlap_correct.py), behind the UMI step and ahead of the adapter
    trimming, which needs both mates uncut.  The overlap is found as the trimming finds it, the largest accepted insert
    length; at a difference inside it a base of ``bad_phred`` or less takes the complement and the quality of the
    mate's base of ``good_phred`` or more, and every other difference is left standing.  The trimming, the read filter,
    the duplicate removal, ``qc``'s "after" stage, ``write_reads`` and the scan then see corrected records: a pair
    that three low-quality miscalls kept from merging merges, and PCR copies that differ by such a miscall are
    duplicates.  Lengths and record indices stay, so names and ``m_original_reads`` are those of the sequencer.  The
    counters gain ``correction_overlapping_pairs``, ``correction_pairs_with_diffs``, ``corrected_reads``,
    ``corrected_bases`` and ``correction_diffs_left`` between the UMI step's keys and the trimming's, the same on every
    route.  ``ValueError`` for anything else.  Without it nothing more is loaded, queued or allocated."""
    return _pair_end_matches(ref_file, fusion_csv, read1_file, read2_file, device, deletion_threshold,
                             remove_alignables, chunk_bytes, ref_chunk_bytes, inflate, tail, originals,
                             alignable_filter, read_filter, adapter_trim, **({"qc": qc} if qc is not None else {}),
                             **({"dedup": dedup} if dedup is not None else {}),
                             **({"umi": umi} if umi is not None else {}),
                             **({"write_reads": write_reads} if write_reads is not None else {}),
                             **({"overlap_correct": overlap_correct} if overlap_correct is not None else {}))[:2]


def scan_pair_end_report(ref_file: str, fusion_csv: str, read1_file: str, read2_file: str, device: int = -1,
                         settings: Settings = None, chunk_bytes: int = None, ref_chunk_bytes: int = None,
                         inflate: str = "host", tail: str = "host", originals: bool = False,
                         remove_alignables: bool = False, *,
                         alignable_filter: str = None, read_filter=None,
                         adapter_trim=None, qc=None, dedup=None, umi=None,
                         write_reads=None, overlap_correct=None) -> Tuple[List[FusionResult], dict]:
    """The whole of ``PairEndScanner::scan`` up to the reporters (pescanner.rs:78-176, :335-337):
    files -> matches -> filter -> per-gene-pair sort -> cluster -> qualified fusions, most
    supported first.  ``report_text`` / ``report_json`` / ``report_html`` of fusion_result.py turn the list into
    the reference's stdout block, JSON file and HTML file.  ``chunk_bytes``, ``ref_chunk_bytes``, ``inflate``,
    ``originals`` (what ``report_html`` shows under the supporting reads), ``remove_alignables`` (the reference's last
    filter as it is), ``alignable_filter`` (a last filter that works), ``read_filter`` (a quality filter ahead of the
    scan), ``adapter_trim`` (adapter trimming ahead of that), ``qc`` (the reads measured before and behind the two),
    ``dedup`` (duplicate pairs removed behind the read filter), ``umi`` (UMIs cut off ahead of the trimming and keyed
    into ``dedup``), ``write_reads`` (the cleaned pairs written out as FASTQ files, streamed routes only),
    ``overlap_correct`` (bases inside the pair overlap corrected from the mate, ahead of the trimming): see
    ``scan_pair_end_files``.  ``tail``: "device" also
    clusters in bulk — the first fit of all groups in one host call, the refined breaks of all matches in one
    ``gf_rp_adjust_device`` call (report_tail.py); the same results, counters and report bytes."""
    settings = settings or Settings()
    return report_matches(*_pair_end_matches(ref_file, fusion_csv, read1_file, read2_file, device,
                                             settings.deletion_threshold, remove_alignables, chunk_bytes,
                                             ref_chunk_bytes, inflate, tail, originals, alignable_filter,
                                             read_filter, adapter_trim, **({"qc": qc} if qc is not None else {}),
                                             **({"dedup": dedup} if dedup is not None else {}),
                                             **({"umi": umi} if umi is not None else {}),
                                             **({"write_reads": write_reads} if write_reads is not None else {}),
                                             **({"overlap_correct": overlap_correct} if overlap_correct is not None else {})),
                          settings, tail, device)


def _single_end_matches(ref_file, fusion_csv, read1_file, device, deletion_threshold, route, chunk_bytes,
                        ref_chunk_bytes=None, inflate="host", tail="host", originals=False, alignable_filter=None,
                        read_filter=None, adapter_trim=None, *, qc=None, dedup=None, umi=None, write_reads=None,
                        overlap_correct=None):
    """(matches kept, counters, fusions, fusion sequences): ``scan_single_end_files`` and what the report needs."""
    if write_reads is not None:   # (checked first)
        from .read_write import need_read_writer
        need_read_writer(write_reads)
    from .adapter_trim import need_adapter_trim
    from .dedup import need_dedup
    from .read_filter import need_read_filter
    from .read_qc import need_read_qc
    from .report_tail import need_tail
    from .umi import need_umi
    need_tail(tail)
    need_read_filter(read_filter)
    need_read_qc(qc)
    need_dedup(dedup)
    if need_umi(umi) is not None:
        umi.need_sides(1)
    from .overlap_correct import need_pairs
    need_pairs(overlap_correct, False)
    if write_reads is not None:
        write_reads.need_route((read1_file,), umi, chunk_bytes is not None)
    if need_adapter_trim(adapter_trim) is not None and not adapter_trim.adapter_r1:
        raise ValueError("adapter_trim: single-end reads are trimmed by sequence, and this one has no adapter_r1")
    _need_whole_contigs(alignable_filter, False, ref_chunk_bytes)
    if route not in ("device", "host"):
        raise ValueError("route must be 'device' or 'host', not %r" % (route,))
    if chunk_bytes is not None and route != "device":
        raise ValueError("chunk_bytes streams the file through the device route; route=%r reads it whole" % (route,))
    fq_inflate, ref_inflate = _route_inflate(inflate, chunk_bytes, ref_chunk_bytes)
    with open_index(ref_file, fusion_csv, device, ref_chunk_bytes, ref_inflate) as (ix, fusions):
        mapper = FusionMapper(ix)
        if chunk_bytes is not None:
            produced = streamed_found(ix, mapper, (read1_file,), chunk_bytes, fq_inflate, originals,
                                      **({"read_filter": read_filter} if read_filter is not None else {}),
                                      **({"adapter_trim": adapter_trim} if adapter_trim is not None else {}),
                                      **({"qc": qc} if qc is not None else {}),
                                      **({"dedup": dedup} if dedup is not None else {}),
                                      **({"umi": umi} if umi is not None else {}),
                                      **({"write_reads": write_reads} if write_reads is not None else {}),
                                      **({"overlap_correct": overlap_correct} if overlap_correct is not None else {}))
        else:   # (both routes start from the records in HBM, where the read filter runs)
            b, text = FastqReader(read1_file).read_all_device(ix)
            measured_reads(ix, qc, "before", b)
            (b,), codes, tagged = tagged_reads(ix, umi, text, b)
            (b,), trimmed = trimmed_reads(ix, adapter_trim, b)
            (b,), counted = filtered_reads(ix, read_filter, b)
            (b,), deduplicated = deduplicated_reads(ix, dedup, b, **({} if codes is None else {"umi_codes": codes}))
            if adapter_trim is not None or read_filter is not None or dedup is not None or _cuts(umi):
                measured_reads(ix, qc, "after", b)
            if route == "device":
                produced = deduplicated(counted(trimmed(tagged(single_end_found(ix, mapper, b, text, originals)))))
            else:
                produced = deduplicated(counted(trimmed(tagged(_single_end_host_found(mapper, b, text, originals)))))
        kept, counters = finish_matches(produced[0], mapper, deletion_threshold, False, *produced[1:], tail=tail,
                                        alignable_filter=alignable_filter)
        return kept, counters, fusions, list(ix.m_fusion_seq)


def scan_single_end_files(ref_file: str, fusion_csv: str, read1_file: str, device: int = -1,
                          deletion_threshold: int = 50, route: str = "device",
                          chunk_bytes: int = None, ref_chunk_bytes: int = None,
                          inflate: str = "host", tail: str = "host",
                          originals: bool = False, *, alignable_filter: str = None,
                          read_filter=None, adapter_trim=None, qc=None,
                          dedup=None, umi=None, write_reads=None,
                          overlap_correct=None) -> Tuple[List[ReadMatch], dict]:
    """``SingleEndScanner`` (src/core/sescanner.rs:62-195) up to the sorted, filtered match list:
    every read is mapped, then its reverse complement when it was mapable without a match.

    ``route="device"``: the records stay in HBM from the FASTQ cut to the hit list — one ``gf_se_scan_device`` call
    (single_end.py), the tail by ``finish_pair_hits``; the counters add ``retried_reads``.  ``route="host"``: the
    records go to the host and through ``FusionMapper.scan_single_end`` (two mapping calls over host buffers, the tail
    per matched read).  Both give the same matches and counters.

    ``chunk_bytes`` (device route only): None reads the file whole; with a value it is streamed in chunks of that many
    bytes of plain text (scan_stream.scan_single_text_stream), as in ``scan_pair_end_files``; the counters add
    ``chunks``.  ``ref_chunk_bytes`` (either route): the reference FASTA in chunks, see ``scan_pair_end_files``.
    ``inflate``: where the streamed ``.gz`` files are inflated, see ``scan_pair_end_files``.  ``tail``: where the
    filters and the sort run, see ``scan_pair_end_files``.  ``originals``: every match carries its read's FASTQ
    record in ``m_original_reads``, on every route; see ``scan_pair_end_files``.  ``alignable_filter``: None or
    "genome", the whole-genome alignable filter on the device; see ``scan_pair_end_files``.  ``read_filter``: None or a
    ``ReadFilter``, the quality filter ahead of the scan, on either route; see ``scan_pair_end_files``.
    ``adapter_trim``: None or an ``AdapterTrim`` with ``adapter_r1``, adapter trimming by sequence ahead of that, on
    either route; ``ValueError`` without ``adapter_r1``; see ``scan_pair_end_files``.  ``qc``: None or a ``ReadQc``,
    the reads measured before and behind the two, on either route (no insert sizes: there are no pairs); see
    ``scan_pair_end_files``.  ``dedup``: None or a ``Dedup``, duplicate reads removed behind the read filter, on either
    route; see ``scan_pair_end_files``.  ``umi``: None or a ``Umi``, the reads' UMIs cut off ("read1", or "per_read",
    which is the same here) or read from their names ("name") ahead of the trimming and keyed into ``dedup``, on either
    route; ``ValueError`` for "read2"; see ``scan_pair_end_files``.  ``write_reads``: None or a ``ReadWriter`` without
    ``out2``, the reads that still have bases written to ``out1``, with ``chunk_bytes`` only; see
    ``scan_pair_end_files``.  ``overlap_correct``: anything but None raises ``ValueError``, an ``OverlapCorrect`` too:
    the correction needs pairs."""
    return _single_end_matches(ref_file, fusion_csv, read1_file, device, deletion_threshold, route, chunk_bytes,
                               ref_chunk_bytes, inflate, tail, originals, alignable_filter, read_filter,
                               adapter_trim, **({"qc": qc} if qc is not None else {}),
                               **({"dedup": dedup} if dedup is not None else {}),
                               **({"umi": umi} if umi is not None else {}),
                               **({"write_reads": write_reads} if write_reads is not None else {}),
                             **({"overlap_correct": overlap_correct} if overlap_correct is not None else {}))[:2]


def scan_single_end_report(ref_file: str, fusion_csv: str, read1_file: str, device: int = -1,
                           settings: Settings = None, route: str = "device", chunk_bytes: int = None,
                           ref_chunk_bytes: int = None, inflate: str = "host",
                           tail: str = "host", originals: bool = False, *,
                           alignable_filter: str = None, read_filter=None,
                           adapter_trim=None, qc=None, dedup=None, umi=None,
                           write_reads=None, overlap_correct=None) -> Tuple[List[FusionResult], dict]:
    """``SingleEndScanner::scan`` up to the reporters: files -> qualified fusions.  ``route``, ``chunk_bytes``,
    ``ref_chunk_bytes``, ``inflate``, ``originals``, ``alignable_filter``, ``read_filter``, ``adapter_trim``, ``qc``, ``dedup``,
    ``umi``, ``write_reads``, ``overlap_correct``: see
    ``scan_single_end_files``; ``tail``: see
    ``scan_pair_end_report``."""
    settings = settings or Settings()
    return report_matches(*_single_end_matches(ref_file, fusion_csv, read1_file, device, settings.deletion_threshold,
                                               route, chunk_bytes, ref_chunk_bytes, inflate, tail, originals,
                                               alignable_filter, read_filter, adapter_trim,
                                               **({"qc": qc} if qc is not None else {}),
                                               **({"dedup": dedup} if dedup is not None else {}),
                                               **({"umi": umi} if umi is not None else {}),
                                               **({"write_reads": write_reads} if write_reads is not None else {}),
                                             **({"overlap_correct": overlap_correct} if overlap_correct is not None else {})),
                          settings, tail, device)
