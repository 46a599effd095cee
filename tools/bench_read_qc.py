#!/usr/bin/env python3
"""The read QC (genefuserust_amd/read_qc.py, libgfqc.so) on the 1 M-pair FASTQ pair of tools/bench_read_filter.py (its
generator and its rewrite: a pair in four touched):

    the stats call alone, all four side tables   before R1, R2 and — over what the read filter leaves — after R1, R2;
                                                  GB/s over 2 bytes per base
    the insert call alone                        seconds and pairs per second
    the yardsticks, in the same run              the read filter call with its defaults, and the adapter trimming call
                                                  with the overlap only, on the same input; the compared calls alternate
                                                  round by round, and the median round counts
    the streamed pair scan, with and without     seconds from pinned host text to the hit records

One JSON document on stdout and, with --out, in a file (profiles/read_qc_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_frontend import make_text  # noqa: E402
from tools.bench_read_filter import L, device_seconds, rewrite  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="calls in the timed window of a device call")
    ap.add_argument("--rounds", type=int, default=5, help="rounds in which the compared calls alternate")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd.adapter_trim import AdapterTrim, trim_adapters_device
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
    from genefuserust_amd.read_qc import INSERT_WORDS, SIDE_WORDS, QcResult, ReadQc, qc_insert_device, qc_stats_device
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    from genefuserust_amd.stream import pinned_empty
    dev = torch.device("cuda", 0)
    genes = synth.make_geneset("IDX-D")
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    n = a.pairs
    pr = synth.make_pairs(genes, n, read_len=L, seed=20240302, device="cuda")
    rewrite(pr, n)
    texts = [make_text(b, q, n, L, mate, dev)
             for mate, (b, q) in enumerate(((pr.l_bases, pr.l_quals), (pr.r_bases, pr.r_quals)), 1)]
    del pr
    out = {"tool": "tools/bench_read_qc.py",
           "input": {"pairs": n, "read_len": L, "shape": "IDX-D", "touched": "5 pairs in 20",
                     "text_bytes": int(texts[0].numel() + texts[1].numel())},
           "stats_kernel_variant": "a wavefront a record, a byte a lane (lane = cycle mod 64), counts in registers; "
                                   "the 16-byte-chunk and the 4-cycles-a-lane variants were not built"}
    before = [fastq_cut_device(ix, t) for t in texts]
    after = list(filter_reads_device(ix, ReadFilter(), *before)[:2])
    torch.cuda.synchronize()
    tables = torch.zeros(4, SIDE_WORDS, dtype=torch.int64, device=dev)
    hist = torch.zeros(INSERT_WORDS, dtype=torch.int64, device=dev)

    def stats_before():
        for k, b in enumerate(before):
            qc_stats_device(ix, b, tables[k])

    def stats_all():
        for k, b in enumerate(before + after):
            qc_stats_device(ix, b, tables[k])
    calls = {"stats_call_four_tables": stats_all,
             "stats_call_before_tables": stats_before,
             "insert_call": lambda: qc_insert_device(ix, before[0], before[1], hist),
             "read_filter_call_defaults": lambda: filter_reads_device(ix, ReadFilter(), *before),
             "trim_call_overlap_only": lambda: trim_adapters_device(ix, AdapterTrim(), *before)}
    seconds = {name: [] for name in calls}
    for _ in range(a.rounds):   # the compared calls alternate
        for name, fn in calls.items():
            seconds[name].append(device_seconds(fn, a.steps))
    med = {name: statistics.median(s) for name, s in seconds.items()}
    stage_bytes = int(2 * sum(b.bases.numel() for b in before))
    tables.zero_()
    hist.zero_()
    stats_all()
    calls["insert_call"]()
    torch.cuda.synchronize()
    t = tables.cpu().numpy()
    result = QcResult((t[0], t[1]), (t[2], t[3]), hist.cpu().numpy())
    summary = {stage: result.summary(stage) for stage in ("before", "after")}
    all_bytes = 2 * (summary["before"]["total_bases"] + summary["after"]["total_bases"])
    for name in calls:
        out[name] = {"seconds": med[name], "rounds": seconds[name], "calls_timed": a.steps}
    out["stats_call_four_tables"].update(
        bases_plus_quals_GBps=all_bytes / med["stats_call_four_tables"] / 1e9, bytes=all_bytes,
        relative_to_read_filter_call=med["stats_call_four_tables"] / med["read_filter_call_defaults"], summary=summary)
    out["stats_call_before_tables"].update(
        bases_plus_quals_GBps=stage_bytes / med["stats_call_before_tables"] / 1e9, bytes=stage_bytes,
        relative_to_read_filter_call=med["stats_call_before_tables"] / med["read_filter_call_defaults"])
    inserts = result.insert_size()
    out["insert_call"].update(pairs_per_second=n / med["insert_call"],
                              relative_to_trim_call_overlap_only=med["insert_call"] / med["trim_call_overlap_only"],
                              peak=inserts["peak"], unknown=inserts["unknown"],
                              pairs_with_an_insert=int(sum(inserts["histogram"][1:])))
    del before, after

    pinned = []
    for t in texts:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del texts
    torch.cuda.empty_cache()
    streamed = {"without_qc": [], "with_qc": []}
    for k in range(1 + a.rounds):   # (round 0 warms both up)
        for name in streamed:
            kw = {"qc": ReadQc()} if name == "with_qc" else {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            records = chunks = 0
            for chunk in scan_pair_source_stream(ix, ArraySource(pinned[0]), ArraySource(pinned[1]), a.chunk_mb << 20,
                                                 max_read_len=None, **kw):
                records += int(chunk[0].shape[0])
                chunks += 1
            if kw:
                measured = kw["qc"].result().summary("before")["total_reads"]
            spent = time.perf_counter() - t0
            if k:
                streamed[name].append(spent)
    out["streamed_pair_scan"] = {name: {"seconds": statistics.median(s), "rounds": s} for name, s in streamed.items()}
    out["streamed_pair_scan"].update(chunk_bytes=a.chunk_mb << 20, hit_records=records, chunks=chunks,
                                     reads_measured=measured)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
