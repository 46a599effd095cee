#!/usr/bin/env python3
"""The correction inside the pair overlap (genefuserust_amd/overlap_correct.py, libgfcorrect.so) on the 1 M pairs of
tools/bench_adapter_trim.py — 150-base reads over fragments of N(166, 40) bases clipped to [40, 400] cut from the genes
of the IDX-D shape, TruSeq adapters and random bases behind a short fragment, one base in 200 flipped — with the flipped
bases given the quality '#' (phred 2, below ``bad_phred``) and every other base 'F':

    the correct call in place                   seconds and pairs per second; the input is restored before every call
    the clone alone                             what ``inplace=False`` adds: bases and qualities of both sides copied
    the trimming call with the overlap only     the yardstick: the parent's gf_at_trim_device on the same input, which
                                                does the same search and a gather on top
    the streamed pair scan                      without the keyword, with it, and with ``adapter_trim`` on top; the same
                                                three with ``Dedup``: seconds, ``merged_pairs``, ``dedup_duplicates``
    the model of the predicate on the host      tests/overlap_correct_model.py over the first pairs, and the same totals

The three device calls alternate, round after round, in one run; a call is timed by a device event on either side of
it, and the medians over the rounds are reported beside every round's figures.  One JSON document on stdout and, with
--out, in a file (profiles/overlap_correct_bench.json).

``--resource-usage`` needs no GPU: it compiles gf_overlap_correct.hip as ``make -C genefuserust_amd/scan_csrc
resource-usage`` does, takes the registers, LDS and scratch of ``gf_oc_k_correct`` from the compiler's remarks and puts
them into the document at --out as ``kernel_resource_usage``, beside whatever a measured run left there."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_adapter_trim import L, make_reads  # noqa: E402
from tools.bench_frontend import make_text  # noqa: E402


def call_seconds(prepare, fn, steps):
    """The mean device time of ``fn()`` over ``steps`` calls, each between two events, ``prepare()`` ahead of each."""
    prepare()
    fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(steps):
        prepare()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in pairs) / 1e3 / steps


def resource_usage():
    """What the compiler says of gf_oc_k_correct, with the Makefile's flags: no GPU is needed."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "genefuserust_amd", "scan_csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "gf_overlap_correct.hip"],
                          cwd=here, capture_output=True, text=True, check=True)
    block = done.stderr[done.stderr.index("Function Name: _Z15gf_oc_k_correct"):]
    take = lambda name: int(re.search(re.escape(name) + r": (\d+)", block).group(1))   # noqa: E731
    return {"kernel": "gf_oc_k_correct<16>", "arch": "gfx950", "vgprs": take("VGPRs"), "sgprs": take("TotalSGPRs"),
            "scratch_bytes_per_lane": take("ScratchSize [bytes/lane]"), "lds_bytes_per_block": take("LDS Size [bytes/block]"),
            "occupancy_waves_per_simd": take("Occupancy [waves/SIMD]")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10, help="calls in one round of a device call")
    ap.add_argument("--rounds", type=int, default=5, help="rounds in which the compared calls alternate")
    ap.add_argument("--model-pairs", type=int, default=2_000, help="pairs the host model is run on")
    ap.add_argument("--out", default="")
    ap.add_argument("--resource-usage", action="store_true", help="no measurement: the kernel's registers, LDS and "
                    "scratch from the compiler, merged into the document at --out")
    a = ap.parse_args()
    if a.resource_usage:
        doc = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {"tool": "tools/bench_overlap_correct.py"}
        doc["kernel_resource_usage"] = resource_usage()
        text = json.dumps(doc, indent=1)
        print(json.dumps(doc["kernel_resource_usage"], indent=1))
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd.adapter_trim import AdapterTrim, adapter_totals_counters, trim_adapters_device
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.dedup import Dedup
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.overlap_correct import OverlapCorrect, correct_overlaps_device, correct_totals_counters
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    from genefuserust_amd.stream import pinned_empty
    from tests.overlap_correct_model import Settings, correct_batch
    dev = torch.device("cuda", 0)
    genes = synth.make_geneset("IDX-D")
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    n = a.pairs
    r1, r2, F, flips = make_reads(genes, n, 20240401, dev, with_flips=True)
    quals = [torch.where(f, torch.tensor(ord("#"), dtype=torch.uint8, device=dev),
                         torch.tensor(ord("F"), dtype=torch.uint8, device=dev)).contiguous() for f in flips]
    texts = [make_text(b, q, n, L, mate, dev) for mate, (b, q) in enumerate(zip((r1, r2), quals), 1)]
    m = min(a.model_pairs, n)
    host_reads = [[(bytes(row), bytes(qrow)) for row, qrow in zip(side[:m].cpu().numpy(), q[:m].cpu().numpy())]
                  for side, q in zip((r1, r2), quals)]
    out = {"tool": "tools/bench_overlap_correct.py",
           "input": {"pairs": n, "read_len": L, "shape": "IDX-D", "fragments": "N(166, 40) clipped to [40, 400]",
                     "read_through_pairs": int((F < L).sum()), "flipped": "1 base in 200, quality '#'; the others 'F'",
                     "text_bytes": int(texts[0].numel() + texts[1].numel())}}
    del r1, r2, quals, flips
    batches = [fastq_cut_device(ix, t) for t in texts]
    pristine = [(b.bases.clone(), b.quals.clone()) for b in batches]
    torch.cuda.synchronize()

    def restore():
        for b, (bases, q) in zip(batches, pristine):
            b.bases.copy_(bases)
            b.quals.copy_(q)

    cfg, overlap_only = OverlapCorrect(), AdapterTrim()
    calls = {"correct_in_place": (restore, lambda: correct_overlaps_device(ix, cfg, *batches, inplace=True)),
             "clone_alone": (lambda: None, lambda: [(b.bases.clone(), b.quals.clone()) for b in batches]),
             "trim_call_overlap_only": (lambda: None, lambda: trim_adapters_device(ix, overlap_only, *batches))}
    fresh = correct_overlaps_device(ix, cfg, *batches)[2].cpu().tolist()   # (before any call in place)
    rounds = {name: [] for name in calls}
    for _ in range(a.rounds):   # the compared calls alternate
        for name, (prepare, fn) in calls.items():
            rounds[name].append(call_seconds(prepare, fn, a.steps))
    restore()
    for name, seconds in rounds.items():
        t = statistics.median(seconds)
        out[name] = {"seconds": t, "pairs_per_second": n / t, "rounds": seconds, "calls_per_round": a.steps}
    totals = correct_overlaps_device(ix, cfg, *batches)[2].cpu().tolist()
    out["correct_in_place"]["totals"] = dict(pairs=totals[0], **correct_totals_counters(totals))
    out["correct_in_place"]["same_totals_behind_the_timed_calls"] = totals == fresh   # (every restore was whole)
    trim_totals = trim_adapters_device(ix, overlap_only, *batches)[2].cpu().tolist()
    out["trim_call_overlap_only"]["totals"] = dict(reads=trim_totals[0], **adapter_totals_counters(trim_totals))
    out["correct_over_trim_ratio"] = out["correct_in_place"]["seconds"] / out["trim_call_overlap_only"]["seconds"]
    out["correct_with_clone_over_trim_ratio"] = (out["correct_in_place"]["seconds"] + out["clone_alone"]["seconds"]) / \
        out["trim_call_overlap_only"]["seconds"]

    # the model on the host, and the device on the same pairs
    first = [b._replace(offsets=b.offsets[:m + 1].contiguous(), n_records=m) for b in batches]
    got = correct_overlaps_device(ix, cfg, *first)[2].cpu().tolist()
    t0 = time.perf_counter()
    want = correct_batch(host_reads[0], host_reads[1], Settings()).totals
    out["model_on_host"] = {"pairs": m, "seconds": time.perf_counter() - t0, "same_totals": want == got}
    print("model: %d pairs in %.1f s, same totals: %s" % (m, out["model_on_host"]["seconds"], want == got),
          file=sys.stderr, flush=True)
    del batches, first, pristine

    pinned = []
    for t in texts:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del texts
    torch.cuda.empty_cache()
    with_sequence = AdapterTrim(adapter_r1="illumina", adapter_r2="illumina")
    routes = (("without", {}), ("with_overlap_correct", {"overlap_correct": cfg}),
              ("with_overlap_correct_and_adapter_trim", {"overlap_correct": cfg, "adapter_trim": with_sequence}),
              ("adapter_trim_alone", {"adapter_trim": with_sequence}))
    streamed = {}
    for dedup in (False, True):
        for name, kw in (("warm_up", routes[2][1]),) + routes:
            if dedup:
                kw = dict(kw, dedup=Dedup())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            records = chunks = merged = duplicates = 0
            for chunk in scan_pair_source_stream(ix, ArraySource(pinned[0]), ArraySource(pinned[1]), a.chunk_mb << 20,
                                                 max_read_len=None, **kw):
                records += int(chunk[0].shape[0])
                merged += int(chunk[4]["merged_pairs"])
                duplicates += int(chunk[4].get("dedup_duplicates", 0))
                chunks += 1
            streamed[name + ("_dedup" if dedup else "")] = dict(
                {"seconds": time.perf_counter() - t0, "hit_records": records, "merged_pairs": merged, "chunks": chunks},
                **({"dedup_duplicates": duplicates} if dedup else {}))
    del streamed["warm_up"], streamed["warm_up_dedup"]
    out["streamed_pair_scan"] = dict(streamed, chunk_bytes=a.chunk_mb << 20)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
