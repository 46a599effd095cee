#!/usr/bin/env python3
"""The adapter trimming (genefuserust_amd/adapter_trim.py, libgfadapt.so) on 1 M pairs of 150-base reads shaped like a
cell-free DNA panel: fragments of N(166, 40) bases clipped to [40, 400] cut from the genes of the IDX-D shape, the
TruSeq adapters and then random bases behind a fragment shorter than the reads, one base in 200 flipped:

    the trimming call alone                     overlap only, and overlap + sequence; seconds and pairs per second
    the read filter call on the same input      the yardstick: gf_pp_filter_device with its default settings
    the streamed pair scan, with and without    seconds from pinned host text to the hit records
    the model of the predicate on the host      tests/adapter_trim_model.py over the first pairs, and the same totals

One JSON document on stdout and, with --out, in a file (profiles/adapter_trim_bench.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_frontend import make_text  # noqa: E402
from tools.bench_read_filter import device_seconds  # noqa: E402

L = 150
TRUSEQ = (b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")


def make_reads(genes, n, seed, dev, with_flips=False):
    """(R1 bases, R2 bases) as (n, L) uint8 tensors, and the fragment lengths; ``with_flips``: and, per mate, the (n, L)
    mask of the bases that were flipped."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    G = torch.from_numpy(np.frombuffer(b"".join(genes.seqs), dtype=np.uint8).copy()).to(dev)
    comp = torch.full((256,), ord("N"), dtype=torch.uint8, device=dev)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    F = (166 + 40 * torch.randn(n, device=dev, generator=gen)).round().clamp(40, 400).to(torch.int64)
    start = (torch.rand(n, device=dev, generator=gen) * (G.numel() - 401)).to(torch.int64)
    flip = torch.rand(n, device=dev, generator=gen) < 0.5      # the fragment's strand
    j = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
    out, flips = [], []
    for mate in (0, 1):
        # mate 0 reads the fragment from its start, mate 1 the other strand from its end; on the flipped strand they swap
        forward = flip if mate else ~flip
        inside = j < F[:, None]
        at = torch.where(forward[:, None], start[:, None] + j, (start + F)[:, None] - 1 - j).clamp(0, G.numel() - 1)
        own = G[at]
        own = torch.where(forward[:, None], own, comp[own.long()])
        ad = torch.tensor(list(TRUSEQ[mate]), dtype=torch.uint8, device=dev)
        behind = (j - F[:, None]).clamp(0, L)
        tail = torch.where(behind < ad.numel(), ad[behind.clamp(max=ad.numel() - 1)],
                           acgt[torch.randint(0, 4, (n, L), device=dev, generator=gen)])
        reads = torch.where(inside, own, tail)
        wrong = torch.rand((n, L), device=dev, generator=gen) < 1 / 200
        other = acgt[torch.randint(0, 4, (n, L), device=dev, generator=gen)]
        out.append(torch.where(wrong & (other != reads), other, reads).contiguous())
        flips.append(wrong & (other != reads))
    return (out[0], out[1], F, flips) if with_flips else (out[0], out[1], F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="calls in the timed window of a device call")
    ap.add_argument("--model-pairs", type=int, default=10_000, help="pairs the host model is run on")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd.adapter_trim import AdapterTrim, adapter_totals_counters, trim_adapters_device
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    from genefuserust_amd.stream import pinned_empty
    from tests.adapter_trim_model import Settings, trim_batch
    dev = torch.device("cuda", 0)
    genes = synth.make_geneset("IDX-D")
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    n = a.pairs
    r1, r2, F = make_reads(genes, n, 20240401, dev)
    quals = torch.full((n, L), ord("F"), dtype=torch.uint8, device=dev)
    texts = [make_text(b, quals, n, L, mate, dev) for mate, b in enumerate((r1, r2), 1)]
    m = min(a.model_pairs, n)
    host_reads = [[(bytes(row), b"F" * L) for row in side[:m].cpu().numpy()] for side in (r1, r2)]
    out = {"tool": "tools/bench_adapter_trim.py",
           "input": {"pairs": n, "read_len": L, "shape": "IDX-D", "fragments": "N(166, 40) clipped to [40, 400]",
                     "read_through_pairs": int((F < L).sum()), "flipped": "1 base in 200",
                     "text_bytes": int(texts[0].numel() + texts[1].numel())}}
    del r1, r2, quals
    batches = [fastq_cut_device(ix, t) for t in texts]
    torch.cuda.synchronize()

    overlap_only = AdapterTrim()
    with_sequence = AdapterTrim(adapter_r1="illumina", adapter_r2="illumina")
    s = device_seconds(lambda: filter_reads_device(ix, ReadFilter(), *batches), a.steps)
    out["read_filter_call_defaults"] = {"seconds": s, "pairs_per_second": n / s, "calls_timed": a.steps}
    for name, cfg in (("overlap_only", overlap_only), ("overlap_and_sequence", with_sequence)):
        t = device_seconds(lambda: trim_adapters_device(ix, cfg, *batches), a.steps)
        totals = trim_adapters_device(ix, cfg, *batches)[2].cpu().tolist()
        out["trim_call_" + name] = {"seconds": t, "pairs_per_second": n / t, "calls_timed": a.steps,
                                    "relative_to_read_filter_call": t / s,
                                    "totals": dict(reads=totals[0], **adapter_totals_counters(totals))}

    # the model on the host, and the device on the same pairs
    first = [b._replace(offsets=b.offsets[:m + 1].contiguous(), n_records=m) for b in batches]
    for name, cfg, ms in (("overlap_only", overlap_only, Settings()),
                          ("overlap_and_sequence", with_sequence, Settings(adapter_r1=TRUSEQ[0], adapter_r2=TRUSEQ[1]))):
        got = trim_adapters_device(ix, cfg, *first)[2].cpu().tolist()
        t0 = time.perf_counter()
        want = trim_batch(host_reads[0], host_reads[1], ms).totals
        out["model_on_host_" + name] = {"pairs": m, "seconds": time.perf_counter() - t0, "same_totals": want == got}
        print("model %s: %d pairs in %.1f s" % (name, m, out["model_on_host_" + name]["seconds"]), file=sys.stderr, flush=True)
    del batches, first

    pinned = []
    for t in texts:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del texts
    torch.cuda.empty_cache()
    streamed = {}
    for name, kw in (("warm_up", {}), ("warm_up", {"adapter_trim": with_sequence}), ("without_trimming", {}),
                     ("with_trimming", {"adapter_trim": with_sequence})):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        records = chunks = merged = 0
        for chunk in scan_pair_source_stream(ix, ArraySource(pinned[0]), ArraySource(pinned[1]), a.chunk_mb << 20,
                                             max_read_len=None, **kw):
            records += int(chunk[0].shape[0])
            merged += int(chunk[4]["merged_pairs"])
            chunks += 1
        streamed[name] = {"seconds": time.perf_counter() - t0, "hit_records": records, "merged_pairs": merged,
                          "chunks": chunks}
    del streamed["warm_up"]
    out["streamed_pair_scan"] = dict(streamed, chunk_bytes=a.chunk_mb << 20)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
