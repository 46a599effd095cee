#!/usr/bin/env python3
"""The duplicate removal (genefuserust_amd/dedup.py, libgfdedup.so) on the 1 M-pair FASTQ pair of
tools/bench_read_filter.py (its generator and its rewrite) with a stated share of the pairs repeated: pair i with
i % 100 < --repeat-percent (i >= 100) is a copy of an earlier pair that is no copy itself: half of them of the last
pair in front of their hundred, half of one anywhere before.

    keys, insert and remove, alone and together   a fresh table of 4 M slots for every timed insert (emptied inside
                                                   the timed window: a fill of 80 MB, stated separately)
    insert with and without count
    the yardsticks, in the same run               the read filter call with its defaults, and the adapter trimming
                                                   call with the overlap only, on the same input; the compared calls
                                                   alternate round by round, and the median round counts
    the streamed pair scan                        without dedup, with it, and with remove=False
    the model on the host                         tests/dedup_model.py over the first --model-pairs pairs

One JSON document on stdout and, with --out, in a file (profiles/dedup_bench.json)."""
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from tools.bench_frontend import make_text  # noqa: E402
from tools.bench_read_filter import L, device_seconds, rewrite  # noqa: E402


def repeat(pr, n, percent, seed=7):
    """In place: the share of pairs that are copies of an earlier pair, which is itself no copy (pair j with
    j % 100 >= percent).  Returns how many pairs were overwritten."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    i = torch.arange(100, n)
    i = i[i % 100 < percent]
    block = i // 100
    near = block * 100 - 1                                    # the last pair in front of the copy's own hundred
    far = (torch.rand(i.numel(), generator=g) * block).long() * 100 + percent \
        + (torch.rand(i.numel(), generator=g) * (100 - percent)).long()
    src = torch.where(i % 2 == 0, near, far)
    assert bool((src % 100 >= percent).all()) and bool((src < i).all())
    i, src = i.to(pr.l_bases.device), src.to(pr.l_bases.device)
    for t in (pr.l_bases, pr.l_quals, pr.r_bases, pr.r_quals):
        rows = t.view(n, L)
        rows[i] = rows[src]
    return int(i.numel())


def resource_usage():
    """VGPRs and scratch of each gf_dd_k_* kernel, from the compiler's remarks (make resource-usage compiles the same
    file with the same flags)."""
    src = os.path.join(ROOT, "genefuserust_amd", "scan_csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "gf_dedup.hip"],
                          cwd=src, capture_output=True, text=True)
    out, name = {}, None
    for line in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"gf_[a-z]+_k_[a-z_]+", m.group(1))
            name = name.group(0) if name else None
            if name and not name.startswith("gf_dd_"):
                name = None
            if name:
                out.setdefault(name, {})
        for key, label in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                           ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(label, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--repeat-percent", type=int, default=30)
    ap.add_argument("--slots", type=int, default=1 << 22)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="calls in the timed window of a device call")
    ap.add_argument("--rounds", type=int, default=5, help="rounds in which the compared calls alternate")
    ap.add_argument("--model-pairs", type=int, default=20_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd import dedup as dd
    from genefuserust_amd.adapter_trim import AdapterTrim, trim_adapters_device
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    from genefuserust_amd.stream import pinned_empty
    from tests import dedup_model as model
    dev = torch.device("cuda", 0)
    genes = synth.make_geneset("IDX-D")
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    n = a.pairs
    pr = synth.make_pairs(genes, n, read_len=L, seed=20240302, device="cuda")
    rewrite(pr, n)
    copies = repeat(pr, n, a.repeat_percent)
    host = [t.view(n, L)[:a.model_pairs].cpu().numpy() for t in (pr.l_bases, pr.r_bases)]
    texts = [make_text(b, q, n, L, mate, dev)
             for mate, (b, q) in enumerate(((pr.l_bases, pr.l_quals), (pr.r_bases, pr.r_quals)), 1)]
    del pr
    out = {"tool": "tools/bench_dedup.py",
           "input": {"pairs": n, "read_len": L, "shape": "IDX-D", "touched": "5 pairs in 20",
                     "repeated": "%d pairs in 100 are copies of an earlier pair (%d pairs)" % (a.repeat_percent, copies),
                     "text_bytes": int(texts[0].numel() + texts[1].numel()), "slots": a.slots},
           "resource_usage": resource_usage()}
    out["no_kernel_spills"] = all(k.get("scratch_bytes_per_lane") == 0 and k.get("vgpr_spill") == 0
                                  for k in out["resource_usage"].values()) and len(out["resource_usage"]) >= 6
    batches = [fastq_cut_device(ix, t) for t in texts]
    torch.cuda.synchronize()
    totals = torch.zeros(dd.TOTALS, dtype=torch.int64, device=dev)
    tables = {True: dd.empty_table(a.slots, dev, True), False: dd.empty_table(a.slots, dev, False)}
    rec_keys = dd.keys_device(ix, *batches)
    state = {}

    def empty(counted):
        t = tables[counted]
        t.keys.zero_()
        t.first.fill_(dd.NO_INDEX)
        if counted:
            t.count.zero_()

    def insert(counted):
        empty(counted)
        state["slot"] = dd.insert_device(ix, rec_keys, 0, tables[counted], totals)

    def together():
        empty(True)
        keys = dd.keys_device(ix, *batches)
        slot = dd.insert_device(ix, keys, 0, tables[True], totals)
        dd.remove_device(ix, slot, 0, tables[True], totals, *batches)
    insert(True)
    calls = {"keys_call": lambda: dd.keys_device(ix, *batches),
             "table_fill_with_count": lambda: empty(True),
             "insert_call_with_count": lambda: insert(True),
             "insert_call_without_count": lambda: insert(False),
             "remove_call": lambda: dd.remove_device(ix, state["slot"], 0, tables[True], totals, *batches),
             "keys_insert_remove_together": together,
             "read_filter_call_defaults": lambda: filter_reads_device(ix, ReadFilter(), *batches),
             "trim_call_overlap_only": lambda: trim_adapters_device(ix, AdapterTrim(), *batches)}
    seconds = {name: [] for name in calls}
    for _ in range(a.rounds):   # the compared calls alternate
        for name, fn in calls.items():
            if name == "remove_call":
                insert(True)    # (the slots of the table with counts, as remove reads them)
            seconds[name].append(device_seconds(fn, a.steps))
    med = {name: statistics.median(s) for name, s in seconds.items()}
    for name in calls:
        out[name] = {"seconds": med[name], "rounds": seconds[name], "calls_timed": a.steps}
    fill = med["table_fill_with_count"]
    out["insert_call_with_count"]["seconds_less_the_fill"] = med["insert_call_with_count"] - fill
    out["insert_call_without_count"]["note"] = "its fill is of 16 bytes a slot, not 20"
    three = med["keys_insert_remove_together"] - fill
    out["keys_insert_remove_together"].update(
        seconds_less_the_fill=three,
        relative_to_read_filter_call=three / med["read_filter_call_defaults"],
        relative_to_trim_plus_filter_calls=three / (med["read_filter_call_defaults"] + med["trim_call_overlap_only"]),
        pairs_per_second=n / three)
    totals.zero_()
    together()
    torch.cuda.synchronize()
    out["totals_of_one_pass"] = dict(zip(("offered", "hashed", "new_keys", "duplicates", "bases_removed", "failed_probes"),
                                         totals.cpu().tolist()))
    del batches, tables, rec_keys, state

    t0 = time.perf_counter()
    t = model.Table()
    offered = t.offer([(bytes(x), bytes(y)) for x, y in zip(*host)])
    out["model_on_the_host"] = {"pairs": int(host[0].shape[0]), "seconds": time.perf_counter() - t0,
                                "duplicates": offered.totals[3]}

    pinned = []
    for t in texts:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del texts
    torch.cuda.empty_cache()
    streamed = {"without_dedup": [], "with_dedup": [], "with_dedup_count_only": []}
    results = {}
    for k in range(1 + a.rounds):   # (round 0 warms all three up)
        for name in streamed:
            kw = {} if name == "without_dedup" else {"dedup": dd.Dedup(remove=name == "with_dedup", slots=a.slots)}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            records = chunks = 0
            for chunk in scan_pair_source_stream(ix, ArraySource(pinned[0]), ArraySource(pinned[1]), a.chunk_mb << 20,
                                                 max_read_len=None, **kw):
                records += int(chunk[0].shape[0])
                chunks += 1
            if kw:
                r = kw["dedup"].result()
                results[name] = {"checked": r.checked, "unique": r.unique, "duplicates": r.duplicates,
                                 "bases_removed": r.bases_removed, "rate": r.rate(), "slots": kw["dedup"].slots}
            spent = time.perf_counter() - t0
            results.setdefault(name, {})["hit_records"] = records
            if k:
                streamed[name].append(spent)
    out["streamed_pair_scan"] = {name: dict(results[name], seconds=statistics.median(s), rounds=s)
                                 for name, s in streamed.items()}
    out["streamed_pair_scan"].update(chunk_bytes=a.chunk_mb << 20, chunks=chunks)
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
