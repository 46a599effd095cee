#!/usr/bin/env python3
"""The read filter (genefuserust_amd/read_filter.py, libgfprep.so) on a 1 M-pair FASTQ pair from the synthetic
generator, its bases and qualities rewritten by the record's number so that each of the three reasons and both trims
occur (a pair in four is touched):

    the filter call alone                       GB/s of bases plus qualities, both mates
    the full FASTQ cut of the same text         the yardstick for a one-pass byte kernel, in GB/s of text
    the streamed pair scan, with and without    seconds from pinned host text to the hit records
    the same predicate in numpy on the host     seconds, and the same totals

One JSON document on stdout and, with --out, in a file (profiles/read_filter_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_frontend import make_text  # noqa: E402

L = 150
WINDOW, MEAN = 4, 20


def rewrite(pr, n):
    """In place: of every 20 pairs, 0 gets a poly-G tail of 30 on R1, 1 a tail of 40 low qualities on R2, 2 an R1 with
    every other base low, 3 eight N in R2, 4 an R1 that is good for 10 bases only."""
    lb, lq, rb, rq = (t.view(n, L) for t in (pr.l_bases, pr.l_quals, pr.r_bases, pr.r_quals))
    for t in (lq, rq):
        t.fill_(ord("F"))
    k = torch.arange(n, device=lb.device) % 20
    lb[k == 0, L - 30:] = ord("G")
    rq[k == 1, L - 40:] = ord("#")
    lq[k == 2, :] = ord("I")
    lq[k == 2, 1::2] = ord("#")
    rb[k == 3, 60:68] = ord("N")
    lq[k == 4, 10:] = ord("#")


def numpy_filter(b, q, s):
    """The predicate over reads of one length ((n, L) uint8 arrays), vectorised: (kept length, own reason)."""
    n = b.shape[0]
    e1 = np.full(n, L, dtype=np.int32)
    if s.poly_g_min > 0:
        not_g = (b | 0x20) != ord("g")
        t = np.where(not_g.any(axis=1), np.argmax(not_g[:, ::-1], axis=1), L).astype(np.int32)
        e1 = np.where(t >= s.poly_g_min, L - t, L).astype(np.int32)
    e2 = e1.copy()
    phred = np.maximum(q.astype(np.int32) - 33, 0)
    if s.cut_tail_window > 0:
        W = s.cut_tail_window
        S = np.concatenate([np.zeros((n, 1), dtype=np.int32), np.cumsum(phred, axis=1, dtype=np.int32)], axis=1)
        ok = (S[:, W:] - S[:, :-W]) >= W * s.cut_tail_mean          # column j: the end e = W + j
        ok &= (np.arange(W, L + 1, dtype=np.int32)[None, :] <= e1[:, None])
        e2 = np.where(ok.any(axis=1), L - np.argmax(ok[:, ::-1], axis=1), 0).astype(np.int32)
    inside = np.arange(L, dtype=np.int32)[None, :] < e2[:, None]
    x = b | 0x20
    n_bases = (((x != ord("a")) & (x != ord("c")) & (x != ord("g")) & (x != ord("t"))) & inside).sum(axis=1)
    low = ((phred < s.qualified_phred) & inside).sum(axis=1)
    reason = np.where(e2 < s.length_required, 1, np.where(n_bases > s.n_base_limit, 2,
                      np.where(100 * low > s.unqualified_percent * e2, 3, 0))).astype(np.int32)
    return e2, reason


def numpy_totals(l, r, s):
    (le, lr), (re_, rr) = numpy_filter(*l, s), numpy_filter(*r, s)
    failed = (lr != 0) | (rr != 0)
    tot = [2 * len(le), 0, 0, 0, 0, 0, 0, 0]
    for e2, own in ((le, lr), (re_, rr)):
        kept = ~failed
        tot[1] += int(kept.sum())
        tot[2] += int((kept & (e2 < L)).sum())
        tot[3] += int((L - e2)[kept].sum())
        for k in (1, 2, 3):
            tot[3 + k] += int((own == k).sum())
        tot[7] += int((failed & (own == 0)).sum())
    return tot


def device_seconds(fn, steps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="calls in the timed window of the filter call")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device, totals_counters
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    from genefuserust_amd.stream import pinned_empty
    dev = torch.device("cuda", 0)
    genes = synth.make_geneset("IDX-D")
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    n = a.pairs
    pr = synth.make_pairs(genes, n, read_len=L, seed=20240302, device="cuda")
    rewrite(pr, n)
    host_reads = [tuple(t.view(n, L).cpu().numpy() for t in side)
                  for side in ((pr.l_bases, pr.l_quals), (pr.r_bases, pr.r_quals))]
    texts = [make_text(b, q, n, L, mate, dev)
             for mate, (b, q) in enumerate(((pr.l_bases, pr.l_quals), (pr.r_bases, pr.r_quals)), 1)]
    del pr
    text_bytes = int(texts[0].numel() + texts[1].numel())
    out = {"tool": "tools/bench_read_filter.py", "input": {"pairs": n, "read_len": L, "shape": "IDX-D",
                                                           "text_bytes": text_bytes, "touched": "5 pairs in 20"}}

    # the full cut of both texts (it reads its line counts back, so a host clock around it)
    batches = [fastq_cut_device(ix, t) for t in texts]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batches = [fastq_cut_device(ix, t) for t in texts]
    torch.cuda.synchronize()
    cut_s = time.perf_counter() - t0
    out["full_cut"] = {"seconds": cut_s, "text_GBps": text_bytes / cut_s / 1e9}

    read_bytes = int(2 * (batches[0].bases.numel() + batches[1].bases.numel()))
    for name, cfg in (("window_%d" % WINDOW, ReadFilter(cut_tail_window=WINDOW, cut_tail_mean=MEAN)),
                      ("defaults", ReadFilter())):
        s = device_seconds(lambda: filter_reads_device(ix, cfg, *batches), a.steps)
        totals = filter_reads_device(ix, cfg, *batches)[2].cpu().tolist()
        t0 = time.perf_counter()
        want = numpy_totals(*host_reads, cfg)
        host_s = time.perf_counter() - t0
        out["filter_call_" + name] = {
            "seconds": s, "bases_plus_quals_GBps": read_bytes / s / 1e9, "bytes": read_bytes, "calls_timed": a.steps,
            "relative_to_full_cut": cut_s / s, "totals": dict(reads=totals[0], **totals_counters(totals)),
            "numpy_on_host": {"seconds": host_s, "same_totals": want == totals}}
    del batches

    pinned = []
    for t in texts:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del texts
    torch.cuda.empty_cache()
    cfg = ReadFilter(cut_tail_window=WINDOW, cut_tail_mean=MEAN)
    streamed = {}
    for name, kw in (("warm_up", {}), ("warm_up", {"read_filter": cfg}), ("without_filter", {}),
                     ("with_filter", {"read_filter": cfg})):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        records = chunks = 0
        for chunk in scan_pair_source_stream(ix, ArraySource(pinned[0]), ArraySource(pinned[1]), a.chunk_mb << 20,
                                             max_read_len=None, **kw):
            records += int(chunk[0].shape[0])
            chunks += 1
        streamed[name] = {"seconds": time.perf_counter() - t0, "hit_records": records, "chunks": chunks}
    del streamed["warm_up"]
    out["streamed_pair_scan"] = dict(streamed, chunk_bytes=a.chunk_mb << 20)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
