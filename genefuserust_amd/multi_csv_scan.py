"""Multi-CSV mode from files (``FusionScan::scan_per_fusion_csv``, src/core/fusion_scan.rs:62-188): the reference and
the FASTQ records are read once, every fusion CSV of a list file is scanned against them, and each gets its report.

The paired-end scan is cut where the CSV starts to matter (libgfmcsv.so, include/gf_multi_csv.h):
``prepare_pairs_device`` merges the pairs, gathers the reads a scan will map and packs them — once — and
``scan_prepared_pairs_device`` maps, classifies, retries and compacts them per index, into exactly the ``PairScan``
that ``read_pair.scan_pairs_device`` gives, so ``PairScan.download``, ``finish_pair_hits`` and
``finish_pair_hits_device`` take it unchanged.  libgfmcsv.so is a library of its own on top of libgfmatch.so's public
C ABI (genefuserust_amd/scan_csrc/); it is loaded after ``_lib.lib()`` so that both refer to the one libgfmatch.so of this
tree.  No CPU fallback: without the libraries and a GPU every compute call raises.

With ``chunk_bytes`` the FASTQ files are streamed once for all CSVs (``_stream_multi_csv``): scan_stream's chunk loop
with the scan of one chunk against every index plugged in, and the K results handed back in one block (scan_pack.py).

``multi_csv.py`` (the bare mapping of resident reads over ranks) stays as it is; running this file-level scan on
several ranks is not done here (``plan_multi_csv`` says which rank would own which CSV).
"""
from __future__ import annotations

import ctypes as C
import os
from contextlib import ExitStack
from typing import List, NamedTuple, Optional, Sequence, Tuple

from . import _lib
from .fusion_result import FusionResult, Settings, report_html, report_json, write_report
from .indexer import Indexer
from .read_pair import PairScan, companion_scan, gene_reversed_device

MC_LIB_PATH = os.path.join(_lib._HERE, "libgfmcsv.so")

_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
# libgfmcsv.so, loaded (once) after libgfmatch.so.  Raises if it has not been built, or if GFMATCH_LIB names another
# libgfmatch.so than the one libgfmcsv.so links against (two builds of the mapping in one process).
lib, check = _lib.companion(MC_LIB_PATH, "multi-CSV scan", "gf_mc_last_error", {
    "gf_mc_prepared_bytes": (_i64, [_i64, _i64, _i64, _i32]),
    "gf_mc_retry_capacity": (_i64, [_i64]),
    "gf_mc_scan_workspace_bytes": (_i64, [_i64, _i32, _i64]),
    "gf_mc_pairs_prepare_device": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp]),
    "gf_mc_pairs_scan_device": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i32,
                                          _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "gf_mc_last_error": (C.c_char_p, []),
})


class PreparedPairs(NamedTuple):
    """The CSV-independent half of a pair scan, device resident: ``buffer`` is what gf_mc_pairs_prepare_device filled
    (merged lengths and diffs, the read lists and their packed form); the R1 / R2 tensors it was made from travel with
    it, because the scan reads the matched reads' bases and qualities from them."""
    buffer: "object"
    l_bases: "object"
    l_quals: "object"
    l_off: "object"
    r_bases: "object"
    r_quals: "object"
    r_off: "object"
    n: int
    max_read_len: int

    def merged_pairs(self) -> int:
        """Synchronises.  The number of pairs that merged."""
        import torch
        if self.n == 0:
            return 0
        pad = (-self.buffer.data_ptr()) % 256   # (the library aligns the caller's base to 256 bytes)
        return int(self.buffer[pad:pad + 32].view(torch.int64)[2].item())


def prepare_pairs_device(indexer: Indexer, l_bases, l_quals, l_off, r_bases, r_quals, r_off, max_read_len: int,
                         stream=None) -> PreparedPairs:
    """``fast_merge`` of every pair, the reads a scan maps gathered into two contiguous lists (R1 / R2 of the pairs that
    did not merge; the merged reads) and those lists packed — everything of ``PairEndScanner::scan_pair_end`` that
    does not depend on the fusion CSV, once, asynchronously.  ``indexer`` only names the device: the result stays valid
    after it is closed.  Tensors as for ``read_pair.scan_pairs_device``."""
    import torch
    _lib.need_device_tensors("prepare_pairs_device", l_bases, l_quals, l_off, r_bases, r_quals, r_off)
    for t in (l_bases, l_quals, r_bases, r_quals):
        assert t.dtype == torch.uint8 and t.is_contiguous()
    n = l_off.numel() - 1
    assert l_off.dtype == torch.int64 and r_off.dtype == torch.int64 and r_off.numel() == n + 1
    assert l_off.is_contiguous() and r_off.is_contiguous()
    assert l_quals.numel() >= l_bases.numel() and r_quals.numel() >= r_bases.numel()
    L = lib()
    dev = l_bases.device
    nbytes = int(L.gf_mc_prepared_bytes(n, l_bases.numel(), r_bases.numel(), int(max_read_len)))
    buf = _lib.workspace(nbytes, dev, stream)
    check(L.gf_mc_pairs_prepare_device(indexer._handle(), l_bases.data_ptr(), l_quals.data_ptr(), l_off.data_ptr(),
                                       l_bases.numel(), r_bases.data_ptr(), r_quals.data_ptr(), r_off.data_ptr(),
                                       r_bases.numel(), n, int(max_read_len), buf.data_ptr(), nbytes,
                                       _lib.stream_handle(dev, stream)))
    return PreparedPairs(buf, l_bases, l_quals, l_off, r_bases, r_quals, r_off, n, int(max_read_len))


def scan_prepared_pairs_device(indexer: Indexer, prepared: PreparedPairs, pair_id_base: int = 0,
                               hits_cap: Optional[int] = None, bytes_cap: Optional[int] = None, retry_cap: int = 0,
                               stream=None) -> PairScan:
    """The CSV-dependent half over a ``PreparedPairs``: both read lists mapped from the packed form, the direction
    gate, the reverse-complement retries and the ordered compaction, one asynchronous call (gf_mc_pairs_scan_device).
    The result equals ``read_pair.scan_pairs_device`` on the same pairs, byte for byte.  ``retry_cap`` 0: the
    library's default (n / 32: every slot is mapped); totals' overflow bit 1 says when it was too small."""
    L = lib()
    p = prepared
    n, max_len = p.n, p.max_read_len
    dev = p.buffer.device
    hits_cap = max(1024, n // 16) if hits_cap is None else int(hits_cap)
    bytes_cap = hits_cap * 2 * max(max_len, 1) if bytes_cap is None else int(bytes_cap)
    ws_bytes = int(L.gf_mc_scan_workspace_bytes(n, max_len, int(retry_cap)))
    head = (indexer._handle(), p.buffer.data_ptr(), p.l_bases.data_ptr(), p.l_quals.data_ptr(), p.l_off.data_ptr(),
            p.l_bases.numel(), p.r_bases.data_ptr(), p.r_quals.data_ptr(), p.r_off.data_ptr(), p.r_bases.numel(), n,
            max_len, gene_reversed_device(indexer, dev).data_ptr(), len(indexer.m_fusions), int(pair_id_base),
            int(retry_cap))
    return companion_scan(check, L.gf_mc_pairs_scan_device, head, dev, ws_bytes, hits_cap, bytes_cap, stream)


# ---- the list file and the report names -------------------------------------------------------------------------

def read_csv_list(path: str) -> List[str]:
    """``get_fusion_csv_vec_from_input`` (fusion_scan.rs:253-280): the fusion CSVs a list file names, one per line —
    lines trimmed, empty ones skipped, order and duplicates kept.  A named file that does not exist raises
    ``FileNotFoundError`` (the reference prints "Fusion csv file '..' was not found." and exits); a line of more than
    1000 bytes raises ``ValueError`` (the reference's LimitedBufReader panics)."""
    out: List[str] = []
    with open(path, "rb") as f:
        for raw in f:
            if len(raw.rstrip(b"\n")) > 1000:
                raise ValueError("%s: a line of more than 1000 bytes" % path)
            s = raw.decode("utf-8").strip()
            if not s:
                continue
            if not os.path.isfile(s):
                raise FileNotFoundError("Fusion csv file '%s' was not found." % s)
            out.append(s)
    return out


def _rust_stem_ext(path: str) -> Tuple[str, str, Optional[str]]:
    """(parent, file_stem, extension) as std::path::Path gives them: the extension is what follows the LAST dot of
    the file name, and a name that only starts with a dot has none."""
    parent, name = os.path.split(path)
    dot = name.rfind(".")
    if dot <= 0:
        return parent, name, None
    return parent, name[:dot], name[dot + 1:]


def report_names(report_file: str, csv_paths: Sequence[str]) -> List[str]:
    """``get_report_names_from_fusion_csvs`` (fusion_scan.rs:190-251) for one report file: per CSV
    ``<parent>/<stem>_<csvstem>.<ext>``; ``[]`` for an empty ``report_file``.  A report file without an extension raises
    ``ValueError`` (the reference unwraps it)."""
    if not report_file:
        return []
    parent, stem, ext = _rust_stem_ext(report_file)
    if ext is None:
        raise ValueError("report file %r has no extension" % report_file)
    return [os.path.join(parent, "%s_%s.%s" % (stem, _rust_stem_ext(c)[1], ext)) for c in csv_paths]


# ---- the scan from files ------------------------------------------------------------------------------------------

def _stream_multi_csv(indexers, files, chunk_bytes: int, hits_cap: Optional[int] = None, inflate: str = "host",
                      originals: bool = False, *, read_filter=None, adapter_trim=None, qc=None, dedup=None,
                      umi=None, write_reads=None, overlap_correct=None):
    """One streamed pass over the FASTQ ``files`` ((R1, R2) or (reads,)) for all ``indexers``: per index what
    ``scan.streamed_found`` gives for it alone — (matches in push order, counters in front of the filter counts, those
    behind them).  The chunk loop is scan_stream's; what is plugged in is the scan of one chunk's records against
    every index with one hand-back: the cut (the full one: gf_mc_pairs_prepare_device takes the qualities at the bases'
    offsets), pairs prepared once, then per index the scan and the names of its hit records, all queued without a
    synchronisation; ``scan_pack.pack_scans_device`` over the K results; one ``download``.  An index whose scan or
    names did not fit is scanned again alone for that chunk (``scan_stream._scan_alone``, with room for everything).
    ``originals``: the FASTQ records of each index's hit records are gathered behind its scan too and fetched per index,
    beside the block (whose format stays): a read-back or two more per index and chunk.  ``read_filter``: a
    ``ReadFilter``, every chunk's records go through the read filter once, ahead of the pairs' preparation
    (``scan_stream._scan_chunk``); every index reports the same filter totals, in front of its filter counts.
    ``adapter_trim``: an ``AdapterTrim``, the same for the adapter trimming ahead of the read filter; its totals stand in
    front of the read filter's.  ``qc``: a ``ReadQc``, every chunk's records are measured once, before and behind the
    two (``scan_stream._scan_chunk``), never per index.  ``dedup``: a ``Dedup``, every chunk's records are
    deduplicated once, behind the read filter; every index reports the same four totals behind the read filter's.
    ``umi``: a ``Umi``, every chunk's records are tagged once, ahead of the trimming (``scan_stream._scan_chunk``); every
    index reports the same five totals in front of the trimming's.  ``write_reads``: a ``ReadWriter``, every chunk's
    records that are left with bases are written once, whatever the number of indexes; every index reports the same three
    totals behind the duplicate removal's.  ``overlap_correct``: an ``OverlapCorrect``, every chunk's pairs are
    corrected once, between the UMI step and the trimming (``scan_stream._scan_chunk``); every index reports the same
    five totals between theirs."""
    from . import scan_pack, scan_stream
    from .overlap_correct import CORRECT_COUNTER_KEYS
    from .adapter_trim import ADAPTER_COUNTER_KEYS
    from .dedup import DEDUP_COUNTER_KEYS
    from .read_filter import COUNTER_KEYS
    from .fusion_mapper import FusionMapper
    from .read_pair import finish_pair_hits
    from .scan import named_from_device, route_counters
    from .umi import UMI_COUNTER_KEYS
    single = len(files) == 1
    count_key = "reads" if single else "pairs"
    first_caps = {} if hits_cap is None else dict(hits_cap=int(hits_cap))
    mappers = [FusionMapper(ix) for ix in indexers]
    found = [[] for _ in indexers]
    sums = [{count_key: 0, "merged_pairs": 0, "retried_reads": 0} for _ in indexers]
    extra = (() if umi is None else UMI_COUNTER_KEYS) + (() if overlap_correct is None else CORRECT_COUNTER_KEYS) \
        + (() if adapter_trim is None else ADAPTER_COUNTER_KEYS) \
        + (() if read_filter is None else COUNTER_KEYS) + (() if dedup is None else DEDUP_COUNTER_KEYS)
    if write_reads is not None:
        from .read_write import WRITE_COUNTER_KEYS
        extra += WRITE_COUNTER_KEYS
    for t in sums:
        t.update(dict.fromkeys(extra, 0))
    chunks = 0

    def scan_records(ix0, texts, batches, m, done, max_read_len, names):
        reads = scan_stream._chunk_reads(batches, m, max_read_len)
        offs, nb, mrl = reads
        prepared = None
        if not single:
            l, r = batches
            prepared = prepare_pairs_device(ix0, l.bases[:nb[0]], l.quals[:nb[0]], offs[0], r.bases[:nb[1]],
                                            r.quals[:nb[1]], offs[1], mrl)
        # (check_lengths: max_read_len is the chunk's longest read, and waiting for a scan's totals is what this avoids)
        steps = [scan_stream._scan_step(ix, texts, batches, m, done, reads, prepared, check_lengths=False)
                 for ix in indexers]
        scans, gathered, records = [], [], []
        for scan, _, gather, gather_records in steps:
            scans.append(scan(**first_caps))
            gathered.append(gather(scans[-1]))
            if originals:
                records.append(gather_records(scans[-1]))
        out = []
        for k, u in enumerate(scan_pack.pack_scans_device(scans, gathered).download()):
            if u.bits & ~scan_pack.OVER_NAMES:   # the scan itself did not fit (or is not one): again, alone, with room
                if u.bits & scan_pack.BAD_SCAN:
                    raise _lib.GfError(_lib.GF_ERR_ARG, "scan %d of a chunk does not hold together: %r" % (k, u.totals))
                out.append(scan_stream._scan_alone(steps[k], steps[k][1], m, single, True, originals))
                continue
            if u.bits:   # only its names did not fit: gathered again with the size the header asked for
                rec, hb, hq, tot = scans[k].download()
                tot[count_key] = m
                out.append((rec, hb, hq, steps[k][2](scans[k], names_cap=u.name_bytes).download(), tot))
            else:
                out.append((u.rec, u.bases, u.quals, u.names, dict(u.totals, **{count_key: m})))
            if originals:
                out[-1] += (scan_stream.fetch_records(records[k], steps[k][3], scans[k]),)
        return out

    with ExitStack() as opened:
        sources = scan_stream.open_fastq_sources(opened, files, inflate)
        for per_index in scan_stream._scan_source_stream(indexers[0], sources, chunk_bytes, None, True, scan_records,
                                                         lean=False, **({} if read_filter is None else
                                                                        {"read_filter": read_filter}),
                                                         **({} if adapter_trim is None else
                                                            {"adapter_trim": adapter_trim}),
                                                         **({} if qc is None else {"qc": qc}),
                                                         **({} if dedup is None else {"dedup": dedup}),
                                                         **({} if umi is None else {"umi": umi}),
                                                         **({} if write_reads is None else
                                                            {"write_reads": write_reads}),
                                                         **({} if overlap_correct is None else
                                                            {"overlap_correct": overlap_correct})):
            for k, (rec, hb, hq, names, tot, *orig) in enumerate(per_index):
                found[k] += named_from_device(finish_pair_hits(mappers[k], rec, hb, hq), rec, names, *orig)
                for key in sums[k]:
                    sums[k][key] += tot[key]
            chunks += 1
    out = []
    for f, t in zip(found, sums):
        before, after = route_counters(count_key, t[count_key], len(f), t, chunks)
        before.update({k: t[k] for k in extra})
        out.append((f, before, after))
    return out


def scan_multi_csv_report(ref_file: str, csv_list_file: str, read1_file: str, read2_file: str = "", device: int = -1,
                          settings: Settings = None, json_file: str = "", command: str = "", version: str = "",
                          time: str = "", ref_chunk_bytes: int = None, chunk_bytes: int = None,
                          hits_cap: int = None, inflate: str = "host", tail: str = "host", originals: bool = False,
                          html_file: str = "", *, read_filter=None, adapter_trim=None,
                          qc=None, dedup=None, umi=None,
                          write_reads=None, overlap_correct=None) -> List[Tuple[str, List[FusionResult], dict]]:
    """``scan_per_fusion_csv``: ``[(csv_path, results, counters)]`` in list order, each entry what
    ``scan.scan_pair_end_report`` (or, without ``read2_file``, ``scan.scan_single_end_report``) returns for that CSV
    alone: the whole-file routes of scan.py, piece by piece.  The FASTA is read once and the FASTQ cut once; with
    ``read2_file`` the pairs are prepared once, and ``scan.pairs_found`` scans the prepared pairs.  Per CSV:
    parse it, build its index, scan, finish, filter, sort, cluster; the index is closed before the next one.  With
    ``json_file`` each entry's ``report_json`` goes to its ``report_names`` name — two entries with the same stem share
    a name and the later one overwrites the earlier, as in the reference; with ``html_file`` its ``report_html`` goes
    to the name made of that file in the same way, before the JSON.  ``originals``: the matches carry their FASTQ records
    for the HTML report (``scan.scan_pair_end_files``); the streamed mode gathers and fetches them per index, beside
    the one block.  ``ref_chunk_bytes``: None keeps every
    contig of the FASTA on the host for the whole run; with a value one streamed pass over the FASTA cuts the gene
    slices of all CSVs on the device (``ref_cut.cut_gene_slices``), and the results are the same.

    ``chunk_bytes``: None reads the FASTQ files whole and keeps the records resident while one index after the other is
    built, scanned and closed.  With a value the files are streamed once, in chunks of that many bytes of plain text
    (``_stream_multi_csv``): every index is built up front and stays open for the pass — 0.15 GB of HBM for an index of
    the druggable panel's shape, 0.5 GB for one of the cancer panel's, times the number of list entries,
    a CSV named twice counting twice — each chunk is cut and its pairs prepared once, scanned against every index, and
    handed back in one block (scan_pack.py): two read-backs per chunk, however many CSVs.  Neither the host nor HBM
    ever holds a file; results and counters are those of the single-CSV streamed scan of each CSV, ``chunks``
    included.  ``hits_cap`` (streamed only): the record capacity of a chunk's first scan per CSV (default: the
    library's, at least 1024); a CSV with more hits in a chunk is scanned again alone for that chunk.

    ``inflate``: where the streamed ``.gz`` files are inflated — the FASTQ files with ``chunk_bytes``, the reference
    with ``ref_chunk_bytes`` — "host", "auto" or "device": see ``scan.scan_pair_end_files``.  ``tail``: where each
    CSV's filters, sort, clustering and break refinement run — "host" or "device", see ``scan.scan_pair_end_report``.

    ``read_filter``: None or a ``read_filter.ReadFilter``, the quality filter ahead of the scan
    (``scan.scan_pair_end_files``).  It runs once — over the resident records, or once per chunk — ahead of
    ``prepare_pairs_device``, and every CSV reports the same seven filter totals.

    ``adapter_trim``: None or an ``adapter_trim.AdapterTrim``, adapter trimming ahead of the read filter
    (``scan.scan_pair_end_files``), once as well; every CSV reports the same five totals.  Without ``read2_file`` it
    needs ``adapter_r1``.

    ``qc``: None or a ``read_qc.ReadQc``, the reads measured before and behind the two (``scan.scan_pair_end_files``):
    once — over the resident records before the loop over the CSVs, or once per chunk — never per index.

    ``dedup``: None or a ``dedup.Dedup``, duplicate records removed behind the read filter
    (``scan.scan_pair_end_files``): once as well — a list of CSVs is deduplicated once — and every CSV reports the same
    four totals.

    ``umi``: None or a ``umi.Umi``, the UMIs cut off the reads or read from their names ahead of the trimming and
    keyed into ``dedup`` (``scan.scan_pair_end_files``): once as well — a list of CSVs is tagged once — and every CSV
    reports the same five totals.  Without ``read2_file`` "read2" raises ``ValueError``.

    ``write_reads``: None or a ``read_write.ReadWriter``, the cleaned records written out as FASTQ files
    (``scan.scan_pair_end_files``): streamed mode only — ``ValueError`` without ``chunk_bytes`` — and once, however many
    CSVs; every CSV reports the same three totals.

    ``overlap_correct``: None or an ``overlap_correct.OverlapCorrect``, bases inside the overlap of a pair corrected
    from the mate between the UMI step and the trimming (``scan.scan_pair_end_files``): once as well — a list of CSVs
    is corrected once — and every CSV reports the same five totals.  Without ``read2_file`` it raises ``ValueError``:
    the correction needs pairs."""
    if write_reads is not None:   # (checked first)
        from .read_write import need_read_writer
        need_read_writer(write_reads)
    from .adapter_trim import need_adapter_trim
    from .dedup import need_dedup
    from .fastq import FastqReader, FastqReaderPair
    from .umi import need_umi
    from .read_filter import need_read_filter
    from .read_qc import need_read_qc
    from .report_tail import need_tail
    need_tail(tail)
    need_read_filter(read_filter)
    need_read_qc(qc)
    need_dedup(dedup)
    if need_umi(umi) is not None:
        umi.need_sides(2 if read2_file else 1)
    from .overlap_correct import need_pairs
    need_pairs(overlap_correct, bool(read2_file))
    if write_reads is not None:
        write_reads.need_route((read1_file, read2_file) if read2_file else (read1_file,), umi, chunk_bytes is not None)
    if need_adapter_trim(adapter_trim) is not None and not read2_file and not adapter_trim.adapter_r1:
        raise ValueError("adapter_trim: single-end reads are trimmed by sequence, and this one has no adapter_r1")
    from .fusion_mapper import FusionMapper
    from .indexer import Fusion
    from .scan import (GeneSlices, _cuts, _route_inflate, deduplicated_reads, filtered_reads, finish_matches, measured_reads,
                       open_index, pairs_found, read_contigs, report_matches, single_end_found, tagged_reads, trimmed_reads)
    settings = settings or Settings()
    fq_inflate, ref_inflate = _route_inflate(inflate, chunk_bytes, ref_chunk_bytes)
    csvs = read_csv_list(csv_list_file)
    names, html_names = report_names(json_file, csvs), report_names(html_file, csvs)

    def write(k: int, results) -> None:   # (the HTML first: pescanner.rs:340-342)
        if html_names:
            write_report(html_names[k], report_html(results, command, version, time, settings))
        if names:
            with open(names[k], "w") as f:
                f.write(report_json(results, command, version, time, settings))
    if ref_chunk_bytes is None:
        refs = [read_contigs(ref_file)] * len(csvs)
    else:
        from .ref_cut import cut_gene_slices
        refs = [GeneSlices(s) for s in cut_gene_slices(ref_file, [Fusion.parse_csv(c) for c in csvs], ref_chunk_bytes,
                                                       device, ref_inflate)]
    out: List[Tuple[str, List[FusionResult], dict]] = []
    if chunk_bytes is not None:
        with ExitStack() as stack:
            opened = [stack.enter_context(open_index(refs[k], csv, device)) for k, csv in enumerate(csvs)]
            files = (read1_file, read2_file) if read2_file else (read1_file,)
            produced = (_stream_multi_csv([ix for ix, _ in opened], files, chunk_bytes, hits_cap, fq_inflate, originals,
                                          **({} if read_filter is None else {"read_filter": read_filter}),
                                          **({} if adapter_trim is None else {"adapter_trim": adapter_trim}),
                                          **({} if qc is None else {"qc": qc}),
                                          **({} if dedup is None else {"dedup": dedup}),
                                          **({} if umi is None else {"umi": umi}),
                                          **({} if write_reads is None else {"write_reads": write_reads}),
                                          **({} if overlap_correct is None else {"overlap_correct": overlap_correct}))
                        if opened else [])
            for csv, (ix, fusions), (found, before, after) in zip(csvs, opened, produced):
                kept, counters = finish_matches(found, FusionMapper(ix), settings.deletion_threshold, False, before, after,
                                                tail)
                out.append((csv, *report_matches(kept, counters, fusions, list(ix.m_fusion_seq), settings, tail, device)))
        for k, (_, results, _) in enumerate(out):
            write(k, results)
        return out
    reads = prepared = counted = trimmed = deduplicated = tagged = corrected = None
    for k, csv in enumerate(csvs):
        with open_index(refs[k], csv, device) as (ix, fusions):
            if reads is None:   # (the first index names the device the records go to)
                if read2_file:
                    (l, ltext), (r, rtext) = FastqReaderPair.from_paths(read1_file, read2_file).read_all_device(ix)
                    measured_reads(ix, qc, "before", l, r)
                    (l, r), codes, tagged = tagged_reads(ix, umi, ltext, l, r)
                    if overlap_correct is not None:   # (the helper is called only when the step is asked for)
                        from .scan import corrected_reads
                        (l, r), corrected = corrected_reads(ix, overlap_correct, l, r)
                    (l, r), trimmed = trimmed_reads(ix, adapter_trim, l, r)
                    (l, r), counted = filtered_reads(ix, read_filter, l, r)
                    (l, r), deduplicated = deduplicated_reads(ix, dedup, l, r,
                                                              **({} if codes is None else {"umi_codes": codes}))
                    if (adapter_trim is not None or read_filter is not None or dedup is not None or _cuts(umi)
                            or overlap_correct is not None):
                        measured_reads(ix, qc, "after", l, r)
                    reads = (l, ltext), (r, rtext)
                    prepared = prepare_pairs_device(ix, l.bases, l.quals, l.offsets, r.bases, r.quals, r.offsets,
                                                    max(l.max_read_len(), r.max_read_len(), 1))
                else:
                    b, text = FastqReader(read1_file).read_all_device(ix)
                    measured_reads(ix, qc, "before", b)
                    (b,), codes, tagged = tagged_reads(ix, umi, text, b)
                    (b,), trimmed = trimmed_reads(ix, adapter_trim, b)
                    (b,), counted = filtered_reads(ix, read_filter, b)
                    (b,), deduplicated = deduplicated_reads(ix, dedup, b, **({} if codes is None else {"umi_codes": codes}))
                    if adapter_trim is not None or read_filter is not None or dedup is not None or _cuts(umi):
                        measured_reads(ix, qc, "after", b)
                    reads = b, text
            mapper = FusionMapper(ix)
            if read2_file:
                produced = pairs_found(mapper, reads, prepared.max_read_len,
                                       lambda **caps: scan_prepared_pairs_device(ix, prepared, **caps), originals)
            else:
                produced = single_end_found(ix, mapper, *reads, originals)
            produced = tagged(produced)
            if corrected is not None:
                produced = corrected(produced)
            produced = deduplicated(counted(trimmed(produced)))
            kept, counters = finish_matches(produced[0], mapper, settings.deletion_threshold, False, *produced[1:],
                                            tail=tail)
            results, counters = report_matches(kept, counters, fusions, list(ix.m_fusion_seq), settings, tail, device)
        write(k, results)
        out.append((csv, results, counters))
    return out


def scan_report(ref_file: str, fusion_file: str, read1_file: str, read2_file: str = "", device: int = -1,
                settings: Settings = None, json_file: str = "", command: str = "", version: str = "", time: str = "",
                chunk_bytes: int = None, ref_chunk_bytes: int = None, inflate: str = "host", tail: str = "host",
                originals: bool = False, html_file: str = "", route: str = "device", remove_alignables: bool = False, *,
                alignable_filter: str = None, read_filter=None, adapter_trim=None, qc=None, dedup=None,
                umi=None, write_reads=None, overlap_correct=None):
    """The mode switch of ``FusionScan::scan`` (fusion_scan.rs:311-330): a fusion file with the extension ``csv`` goes
    to the single-CSV scanners (``scan.scan_pair_end_report`` with ``read2_file``, else
    ``scan.scan_single_end_report``) and gives their ``(results, counters)``; anything else is a list of CSVs and
    gives ``scan_multi_csv_report``'s list.  ``chunk_bytes`` streams the FASTQ files of the single-CSV scanners
    (``scan.scan_pair_end_files``); for a list of CSVs this switch raises ``ValueError`` — multi-CSV mode streams its
    files through ``scan_multi_csv_report(chunk_bytes=...)``, called directly.  ``ref_chunk_bytes`` streams the reference FASTA in every mode (``scan.open_index``,
    ``scan_multi_csv_report``).  ``inflate``: where the streamed ``.gz`` files are inflated, in every mode
    (``scan.scan_pair_end_files``).  ``tail``: where the report tail runs, in every mode (``scan.scan_pair_end_report``).
    ``originals``: the matches carry their FASTQ records, in every mode (``scan.scan_pair_end_files``).  ``html_file``:
    ``report_html`` goes there, before the JSON, as ``json_file`` does.  ``route``: the single-end scanner's
    (``scan.scan_single_end_files``).  ``remove_alignables``: the paired-end scanner's (``scan.scan_pair_end_files``);
    ``ValueError`` in the other modes, which do not have it.  ``alignable_filter``: None or "genome", the whole-genome
    alignable filter on the device of the single-CSV scanners (``scan.scan_pair_end_files``); ``ValueError`` for a list
    of CSVs.  ``read_filter``: None or a ``read_filter.ReadFilter``, the quality filter ahead of the scan, in every
    mode (``scan.scan_pair_end_files``); it is handed on only when set.  ``adapter_trim``: None or an
    ``adapter_trim.AdapterTrim``, adapter trimming ahead of the read filter, in every mode, handed on only when set.
    ``qc``: None or a ``read_qc.ReadQc``, the reads measured before and behind the two, in every mode, handed on only
    when set; for a list of CSVs the reads are measured once.  ``dedup``: None or a ``dedup.Dedup``, duplicate records
    removed behind the read filter, in every mode, handed on only when set; a list of CSVs is deduplicated once.
    ``umi``: None or a ``umi.Umi``, the UMIs cut off or read from the names ahead of the trimming and keyed into ``dedup``,
    in every mode, handed on only when set; a list of CSVs is tagged once.  ``write_reads``: None or a
    ``read_write.ReadWriter``, the cleaned records written out as FASTQ files by the streamed routes, handed on only
    when set; ``ValueError`` without ``chunk_bytes``.  ``overlap_correct``: None or an
    ``overlap_correct.OverlapCorrect``, bases inside the overlap of a pair corrected from the mate ahead of the
    trimming, in every mode with pairs, handed on only when set; ``ValueError`` without ``read2_file``; a list of CSVs
    is corrected once."""
    from . import scan
    if write_reads is not None:   # (checked first)
        from .read_write import need_read_writer
        need_read_writer(write_reads)
    from .adapter_trim import need_adapter_trim
    from .dedup import need_dedup
    from .alignable import need_filter
    from .read_filter import need_read_filter
    from .read_qc import need_read_qc
    from .umi import need_umi
    filtered = {} if need_read_filter(read_filter) is None else {"read_filter": read_filter}
    if need_adapter_trim(adapter_trim) is not None:
        filtered["adapter_trim"] = adapter_trim
    if need_read_qc(qc) is not None:
        filtered["qc"] = qc
    if need_dedup(dedup) is not None:
        filtered["dedup"] = dedup
    if need_umi(umi) is not None:
        filtered["umi"] = umi
    from .overlap_correct import need_pairs
    if need_pairs(overlap_correct, bool(read2_file)) is not None:
        filtered["overlap_correct"] = overlap_correct
    if write_reads is not None:
        write_reads.need_route((read1_file, read2_file) if read2_file else (read1_file,), umi, chunk_bytes is not None)
        filtered["write_reads"] = write_reads
    if need_filter(alignable_filter, remove_alignables) and _rust_stem_ext(fusion_file)[2] != "csv":
        raise ValueError("alignable_filter: only the scans of one CSV have this filter")
    if remove_alignables and not (_rust_stem_ext(fusion_file)[2] == "csv" and read2_file):
        raise ValueError("remove_alignables: only the paired-end scan of one CSV has this filter")
    if _rust_stem_ext(fusion_file)[2] == "csv":
        if read2_file:
            results, counters = scan.scan_pair_end_report(ref_file, fusion_file, read1_file, read2_file, device, settings,
                                                          chunk_bytes=chunk_bytes, ref_chunk_bytes=ref_chunk_bytes,
                                                          inflate=inflate, tail=tail, originals=originals,
                                                          remove_alignables=remove_alignables,
                                                          alignable_filter=alignable_filter, **filtered)
        else:
            results, counters = scan.scan_single_end_report(ref_file, fusion_file, read1_file, device, settings, route,
                                                            chunk_bytes=chunk_bytes, ref_chunk_bytes=ref_chunk_bytes,
                                                            inflate=inflate, tail=tail, originals=originals,
                                                            alignable_filter=alignable_filter, **filtered)
        if html_file:
            write_report(html_file, report_html(results, command, version, time, settings))
        if json_file:
            with open(json_file, "w") as f:
                f.write(report_json(results, command, version, time, settings))
        return results, counters
    if chunk_bytes is not None:
        raise ValueError("chunk_bytes: this switch keeps the reads of multi-CSV mode resident; call "
                         "scan_multi_csv_report(chunk_bytes=...) to stream them")
    return scan_multi_csv_report(ref_file, fusion_file, read1_file, read2_file, device, settings, json_file, command,
                                 version, time, ref_chunk_bytes, inflate=inflate, tail=tail, originals=originals,
                                 html_file=html_file, **filtered)
