"""The command line: ``python -m genefuserust_amd -1 R1.fq -2 R2.fq -f fusions.csv -r ref.fa``.

The options of the reference (src/argparse.rs) keep their letters and defaults — ``-h`` is the HTML file, help is
``--help`` only — and the flow is that of src/genefuse.rs: the input files are checked, the command line is printed,
the scan runs (``multi_csv_scan.scan_report``: one CSV or a list of them, paired or single-end), the HTML report and
the JSON report are written, the text result is printed, then the closing line.  What this project adds is spelled
out: the device, the streamed routes, where ``.gz`` files are inflated, where the report tail runs, the
whole-genome alignable filter, the adapter trimming, the quality filter and the duplicate removal of the reads ahead of
the scan, the QC report of the reads, and the cleaned reads written out as FASTQ files.
"""
from __future__ import annotations

import argparse
import datetime
import os
import sys
import time
from typing import List, Optional, Sequence

PROG = "genefuserust_amd"


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog=PROG, add_help=False, description="Gene fusion detection from FASTQ files, on an "
                                "AMD GPU.  The options of GeneFuse keep their letters and defaults.")
    p.add_argument("--help", action="help", help="show this message and exit (-h is the HTML file)")
    p.add_argument("-1", "--read1", required=True, help="read1 file name")
    p.add_argument("-2", "--read2", default="", help="read2 file name")
    p.add_argument("-f", "--fusion", required=True, help="fusion file name, in CSV format; any other extension: a list "
                   "of CSV files, one per line, each scanned and reported under its own name")
    p.add_argument("-r", "--ref", required=True, help="reference fasta file name")
    p.add_argument("-u", "--unique", type=int, default=2, help="specify the least supporting read number is required "
                   "to report a fusion, default is 2")
    p.add_argument("-h", "--html", default="genefuse.html", help="file name to store HTML report, default is "
                   "genefuse.html; empty: none")
    p.add_argument("-j", "--json", default="genefuse.json", help="file name to store JSON report, default is "
                   "genefuse.json; empty: none")
    p.add_argument("-t", "--thread", type=int, default=4, help="worker thread number (accepted, unused: the scan runs "
                   "on the device)")
    p.add_argument("-d", "--deletion", type=int, default=50, help="specify the least deletion length of a intra-gene "
                   "deletion to report, default is 50")
    p.add_argument("-D", "--output_deletions", action="store_true", help="long deletions are not output by default, "
                   "enable this option to output them")
    p.add_argument("-U", "--output_untranslated_fusions", action="store_true", help="the fusions that cannot be "
                   "transcribed or translated are not output by default, enable this option to output them")
    own = p.add_argument_group("this project's own switches")
    own.add_argument("--device", type=int, default=-1, help="the GPU to run on, default is the current one")
    own.add_argument("--chunk-bytes", type=int, default=None, help="stream the FASTQ files in chunks of this many bytes "
                     "of plain text; default: read them whole")
    own.add_argument("--ref-chunk-bytes", type=int, default=None, help="stream the reference in chunks of this many "
                     "bytes and cut the gene slices out on the device; default: read it whole on the host")
    own.add_argument("--inflate", choices=("host", "auto", "device"), default="host", help="where streamed .gz files "
                     "are inflated: host; auto: BGZF files on the device; device: BGZF files only")
    own.add_argument("--tail", choices=("host", "device"), default="host", help="where filters, sort, clustering and "
                     "break refinement run")
    own.add_argument("--route", choices=("device", "host"), default="device", help="the single-end scan: on the device, "
                     "or with the records on the host")
    own.add_argument("--remove-alignables", action="store_true", help="apply the reference's last filter (paired-end, "
                     "one CSV, whole reference).  Off by default: the reference's Matcher, as it is, removes nothing on "
                     "a genome and panics on small references")
    own.add_argument("--alignable-filter", choices=("genome",), default=None, help="genome: drop the matches whose read "
                     "lies end to end somewhere in the reference, tested on the device (one CSV, whole reference).  "
                     "Off by default")
    rf = p.add_argument_group("the read filter (off by default; any of its options switches it on)")
    rf.add_argument("--read-filter", action="store_true", help="filter and trim the reads on the device ahead of the "
                    "scan, with the defaults below: poly-G and low-quality tails are cut off, pairs with a mate that "
                    "is too short, holds too many N or too many low bases are not scanned")
    rf.add_argument("--qualified-phred", type=int, default=None, help="a base below this phred is a low base, default 15")
    rf.add_argument("--unqualified-percent", type=int, default=None, help="the share of low bases a read may have, "
                    "default 40")
    rf.add_argument("--n-base-limit", type=int, default=None, help="the most N bases a read may have, default 5")
    rf.add_argument("--length-required", type=int, default=None, help="the shortest read kept, default 15")
    rf.add_argument("--cut-tail-window", type=int, default=None, help="cut a read behind its last window of this many "
                    "bases that reaches --cut-tail-mean; 1 to 64, default 0: off")
    rf.add_argument("--cut-tail-mean", type=int, default=None, help="the mean phred a tail window must reach, default 20")
    rf.add_argument("--poly-g-min", type=int, default=None, help="cut off a poly-G tail of at least this many bases, "
                    "default 10; 0: off")
    at = p.add_argument_group("adapter trimming (off by default; any of its options switches it on)")
    at.add_argument("--trim-adapters", action="store_true", help="cut the reads to the insert on the device ahead of "
                    "the read filter and the scan: pairs by the overlap of their mates, with the defaults below")
    at.add_argument("--adapter-r1", default=None, help="the adapter behind read1's insert, looked for in reads that "
                    "no overlap cut (and in single-end reads, which need it): 4 to 64 bases of ACGT, or illumina")
    at.add_argument("--adapter-r2", default=None, help="the adapter behind read2's insert, as --adapter-r1")
    at.add_argument("--adapter-min-overlap", type=int, default=None, help="the fewest positions an overlap compares, "
                    "default 30")
    at.add_argument("--adapter-max-diff", type=int, default=None, help="the most differences inside an overlap, "
                    "default 5")
    at.add_argument("--adapter-diff-percent", type=int, default=None, help="the share of differences inside an "
                    "overlap, default 20")
    at.add_argument("--adapter-min-match", type=int, default=None, help="the fewest adapter bases looked for at a "
                    "read's end, default 10")
    qc = p.add_argument_group("read QC (off by default)")
    qc.add_argument("--qc-json", default=None, metavar="FILE", help="measure the reads on the device, before and behind "
                    "the adapter trimming and the read filter, and write the QC report there: reads, bases, Q20/Q30, "
                    "GC, per-cycle quality and base content, insert sizes; one file, also for a list of CSV files")
    qc.add_argument("--qc-no-insert-size", action="store_true", help="leave the insert sizes of the pairs out of the "
                    "QC report (needs --qc-json)")
    dd = p.add_argument_group("duplicate removal (off by default; any of its options switches it on)")
    dd.add_argument("--dedup", action="store_true", help="find duplicate pairs (reads) on the device behind the read "
                    "filter, by their bases with the case folded, and scan only the first of each; with --qc-json the "
                    "report gains the duplication rate")
    dd.add_argument("--dedup-count-only", action="store_true", help="count the duplicates, remove none")
    dd.add_argument("--dedup-max-slots", type=int, default=None, metavar="N", help="the largest hash table, a power "
                    "of two of slots of 20 bytes, default 2^31; a table grows to twice the records offered")
    um = p.add_argument_group("unique molecular identifiers (off by default; --umi-loc switches them on)")
    um.add_argument("--umi-loc", choices=("name", "read1", "read2", "per_read"), default=None, help="where the library's "
                    "UMIs are.  read1, read2, per_read: the first --umi-len bases of read1, of read2 or of both, cut off on "
                    "the device with --umi-skip bases of spacer behind them, ahead of the adapter trimming; name: behind "
                    "the last ':' of the read's name.  With --dedup two pairs (reads) are duplicates only when their UMIs "
                    "are equal too")
    um.add_argument("--umi-len", type=int, default=None, metavar="N", help="the bases of an inline UMI, 1 to 32 (needs "
                    "--umi-loc read1, read2 or per_read)")
    um.add_argument("--umi-skip", type=int, default=None, metavar="N", help="the bases of spacer behind an inline UMI, "
                    "cut off with it, 0 to 32, default 0 (needs --umi-loc)")
    oc = p.add_argument_group("correction inside the pair overlap (off by default; any of its options switches it on; "
                              "needs -2)")
    oc.add_argument("--correct-overlap", action="store_true", help="where the mates of a pair overlap, rewrite a "
                    "low-quality base that the mate's high-quality base contradicts from the mate, on the device, ahead "
                    "of the adapter trimming")
    oc.add_argument("--correct-min-overlap", type=int, default=None, metavar="N", help="the fewest positions an overlap "
                    "compares, 8 to 512, default 30")
    oc.add_argument("--correct-max-diff", type=int, default=None, metavar="N", help="the most differences inside an "
                    "overlap, default 5")
    oc.add_argument("--correct-diff-percent", type=int, default=None, metavar="N", help="the share of differences "
                    "inside an overlap, 0 to 100, default 20")
    oc.add_argument("--correct-good-phred", type=int, default=None, metavar="Q", help="the least phred of the base that "
                    "is copied, 0 to 93, default 30")
    oc.add_argument("--correct-bad-phred", type=int, default=None, metavar="Q", help="the most phred of the base that "
                    "is rewritten, below --correct-good-phred, default 15")
    wr = p.add_argument_group("the cleaned reads as FASTQ files (off by default; --out1 switches them on)")
    wr.add_argument("--out1", default=None, metavar="FILE", help="write the reads (of read1) that are left with bases "
                    "behind the steps above there, formatted on the device; .gz: compressed by the host's zlib.  "
                    "Streams the FASTQ files: without --chunk-bytes in chunks of 128 MiB")
    wr.add_argument("--out2", default=None, metavar="FILE", help="the same for read2; needed with -2, and a pair is "
                    "written only when both mates are left with bases (needs --out1)")
    wr.add_argument("--umi-in-name", action="store_true", help="write the inline UMI that --umi-loc read1, read2 or "
                    "per_read cuts off into the names, as :UMI at the end of the first token (needs --out1)")
    wr.add_argument("--out-compression", type=int, default=None, metavar="N", help="zlib's level for .gz outputs, 1 to "
                    "9, default 4 (needs --out1)")
    wr.add_argument("--out-deflate", choices=("host", "device"), default=None, help="who compresses .gz outputs: host, "
                    "the host's zlib (the default), or device, BGZF members deflated on the device, which needs every "
                    "output to end in .gz and takes no --out-compression level (needs --out1)")
    return p


DEFAULT_OUT_CHUNK_BYTES = 128 << 20   # what --out1 streams with when --chunk-bytes is not given


READ_FILTER_OPTIONS = ("qualified_phred", "unqualified_percent", "n_base_limit", "length_required", "cut_tail_window",
                       "cut_tail_mean", "poly_g_min")


def _read_filter(args):
    """The ``ReadFilter`` the options ask for, None when none of them is given; ``ValueError`` for a value out of
    range."""
    given = {k: getattr(args, k) for k in READ_FILTER_OPTIONS if getattr(args, k) is not None}
    if not (args.read_filter or given):
        return None
    from .read_filter import ReadFilter
    return ReadFilter(**given)


# option -> the field of ``AdapterTrim`` it sets
ADAPTER_TRIM_OPTIONS = {"adapter_r1": "adapter_r1", "adapter_r2": "adapter_r2", "adapter_min_overlap": "min_overlap",
                        "adapter_max_diff": "max_diff", "adapter_diff_percent": "diff_percent",
                        "adapter_min_match": "min_adapter"}


def _adapter_trim(args):
    """The ``AdapterTrim`` the options ask for, None when none of them is given; ``ValueError`` for a value out of
    range."""
    given = {f: getattr(args, k) for k, f in ADAPTER_TRIM_OPTIONS.items() if getattr(args, k) is not None}
    if not (args.trim_adapters or given):
        return None
    from .adapter_trim import AdapterTrim
    return AdapterTrim(**given)


def _read_qc(args):
    """The ``ReadQc`` the options ask for, None without ``--qc-json``; ``ValueError`` for ``--qc-no-insert-size``
    without it."""
    if not args.qc_json:
        if args.qc_no_insert_size:
            raise ValueError("--qc-no-insert-size needs --qc-json")
        return None
    from .read_qc import ReadQc
    return ReadQc(insert_size=not args.qc_no_insert_size)


def _dedup(args):
    """The ``Dedup`` the options ask for, None when none of them is given; ``ValueError`` for a value out of range."""
    if not (args.dedup or args.dedup_count_only or args.dedup_max_slots is not None):
        return None
    from .dedup import Dedup
    sizes = {}
    if args.dedup_max_slots is not None:   # (a small limit takes the first size down with it)
        sizes = dict(max_slots=args.dedup_max_slots, slots=min(Dedup().slots, max(args.dedup_max_slots, 1)))
    return Dedup(remove=not args.dedup_count_only, **sizes)


def _umi(args):
    """The ``Umi`` the options ask for, None without ``--umi-loc``; ``ValueError`` for ``--umi-len`` or ``--umi-skip``
    without it, and for a value out of range."""
    if args.umi_loc is None:
        for option, value in (("--umi-len", args.umi_len), ("--umi-skip", args.umi_skip)):
            if value is not None:
                raise ValueError("%s needs --umi-loc" % option)
        return None
    from .umi import Umi
    return Umi(args.umi_loc, **{k: v for k, v in (("length", args.umi_len), ("skip", args.umi_skip)) if v is not None})


# option -> the field of ``OverlapCorrect`` it sets
OVERLAP_CORRECT_OPTIONS = {"correct_min_overlap": "min_overlap", "correct_max_diff": "max_diff",
                           "correct_diff_percent": "diff_percent", "correct_good_phred": "good_phred",
                           "correct_bad_phred": "bad_phred"}


def _overlap_correct(args):
    """The ``OverlapCorrect`` the options ask for, None when none of them is given; ``ValueError`` for a value out of
    range, and without ``-2``: the correction needs pairs."""
    given = {f: getattr(args, k) for k, f in OVERLAP_CORRECT_OPTIONS.items() if getattr(args, k) is not None}
    if not (args.correct_overlap or given):
        return None
    if not args.read2:
        raise ValueError("--correct-overlap needs pairs: give read2 with -2")
    from .overlap_correct import OverlapCorrect
    return OverlapCorrect(**given)


def _read_writer(args):
    """The ``ReadWriter`` the options ask for, None without ``--out1``; ``ValueError`` for one of the other four
    without it, and for a value out of range."""
    if args.out1 is None:
        for option, given in (("--out2", args.out2 is not None), ("--umi-in-name", args.umi_in_name),
                              ("--out-compression", args.out_compression is not None),
                              ("--out-deflate", args.out_deflate is not None)):
            if given:
                raise ValueError("%s needs --out1" % option)
        return None
    from .read_write import ReadWriter
    return ReadWriter(args.out1, args.out2, umi_in_name=args.umi_in_name,
                      **({} if args.out_compression is None else {"compress_level": args.out_compression}),
                      **({} if args.out_deflate is None else {"deflate": args.out_deflate}))


def _missing(args) -> Optional[str]:
    """genefuse.rs:75-84: the first input file that is not there."""
    for f in (args.ref, args.read1, args.read2, args.fusion):
        if f and not os.path.isfile(f):
            return f
    return None


def main(argv: Optional[Sequence[str]] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parser().parse_args(argv)
    missing = _missing(args)
    if missing is not None:   # (before anything touches the device)
        print("ERROR: file '%s' doesn't exist, quit now" % missing, file=sys.stderr)
        return 1
    from . import __version__
    from .fusion_result import Settings, report_text
    from .multi_csv_scan import _rust_stem_ext, scan_multi_csv_report, scan_report
    command = " ".join([PROG] + argv)
    started = time.monotonic()
    print("\n# %s\n" % command)
    settings = Settings(args.unique, args.deletion, args.output_deletions, args.output_untranslated_fusions)
    now = str(datetime.datetime.now().astimezone())
    common = dict(device=args.device, settings=settings, json_file=args.json, html_file=args.html, command=command,
                  version=__version__, time=now, chunk_bytes=args.chunk_bytes, ref_chunk_bytes=args.ref_chunk_bytes,
                  inflate=args.inflate, tail=args.tail, originals=bool(args.html))
    try:
        read_filter = _read_filter(args)
        if read_filter is not None:   # (off: the calls of today)
            common["read_filter"] = read_filter
        adapter_trim = _adapter_trim(args)
        if adapter_trim is not None:
            common["adapter_trim"] = adapter_trim
        qc = _read_qc(args)
        if qc is not None:
            common["qc"] = qc
        dedup = _dedup(args)
        if dedup is not None:
            common["dedup"] = dedup
        umi = _umi(args)
        if umi is not None:
            common["umi"] = umi
        overlap_correct = _overlap_correct(args)
        if overlap_correct is not None:
            common["overlap_correct"] = overlap_correct
        write_reads = _read_writer(args)
        if write_reads is not None:   # (the records are written by the streamed routes)
            common["write_reads"] = write_reads
            if common["chunk_bytes"] is None:
                common["chunk_bytes"] = DEFAULT_OUT_CHUNK_BYTES
        if _rust_stem_ext(args.fusion)[2] != "csv" and common["chunk_bytes"] is not None:
            if args.remove_alignables:
                raise ValueError("remove_alignables: only the paired-end scan of one CSV has this filter")
            if args.alignable_filter is not None:
                raise ValueError("alignable_filter: only the scans of one CSV have this filter")
            out = scan_multi_csv_report(args.ref, args.fusion, args.read1, args.read2, **common)   # (streams its files)
        else:
            out = scan_report(args.ref, args.fusion, args.read1, args.read2, route=args.route,
                              remove_alignables=args.remove_alignables, **common,
                              **({"alignable_filter": args.alignable_filter} if args.alignable_filter else {}))
    except (ValueError, FileNotFoundError) as e:
        print("ERROR: %s" % e, file=sys.stderr)
        return 1
    per_csv: List = [r for _, r, _ in out] if isinstance(out, list) else [out[0]]
    if qc is not None:   # (one file: every CSV of a list saw the same reads, and counts the same trimming and filter)
        from .read_qc import report_json
        counters = (out[0][2] if out else None) if isinstance(out, list) else out[1]
        with open(args.qc_json, "w") as f:
            f.write(report_json(qc.result(), counters, **({} if dedup is None else {"duplication": dedup.result()}),
                                **({} if umi is None else {"umi": umi})))
    for results in per_csv:
        sys.stdout.write(report_text(results))
    print("# genefuse v%s, time used: %s seconds\n" % (__version__, time.monotonic() - started))
    return 0
