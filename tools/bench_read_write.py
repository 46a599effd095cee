#!/usr/bin/env python3
"""The FASTQ output (genefuserust_amd/read_write.py, libgfwrite.so) on the 1 M-pair FASTQ pair of
tools/bench_read_filter.py (its generator and its rewrite) behind the read filter with its defaults.

    the format call, wide       against the read filter call with its defaults on the same input and against the
    the format call, plain      format call with the byte-a-lane gather; the compared calls alternate round by round —
                                a warm round, then --rounds rounds of --steps calls — and the median round counts
    the streamed pair scan      with the read filter, three ways: without the writer, with plain output into a temporary
                                directory, and with .gz output; beside it what this host writes and deflates per second,
                                so that nobody reads a disk or zlib bound as the kernel's
    --trace-only                the two format calls and the filter call alone, --steps times each, for a kernel trace
                                in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_read_write.py
                                --trace-only)

One JSON document on stdout and, with --out, in a file (profiles/read_write_bench.json)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from tools.bench_frontend import make_text  # noqa: E402
from tools.bench_read_filter import L, device_seconds, rewrite  # noqa: E402
from tools.bench_umi import commit  # noqa: E402


def resource_usage():
    """VGPRs and scratch of each gf_rw_k_* kernel, from the compiler's remarks (make resource-usage compiles the same
    file with the same flags)."""
    src = os.path.join(ROOT, "genefuserust_amd", "scan_csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "gf_read_write.hip"],
                          cwd=src, capture_output=True, text=True)
    out, name = {}, None
    for line in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"gf_rw_k_[a-z_]+(ILi\d+ELb[01]E)?", m.group(1))
            name = name.group(0) if name else None
            if name:
                out.setdefault(name, {})
        for key, label in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                           ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)")):
            m = re.search(label, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def host_throughput(sample: bytes, level: int, folder: str) -> dict:
    """What this host writes to ``folder`` and deflates per second, on ``sample`` (a piece of the output text)."""
    t0 = time.perf_counter()
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    packed = c.compress(sample) + c.flush()
    deflate_s = time.perf_counter() - t0
    path = os.path.join(folder, "throughput.bin")
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        f.write(sample)
        f.flush()
        os.fsync(f.fileno())
    write_s = time.perf_counter() - t0
    os.unlink(path)
    return {"sample_bytes": len(sample), "zlib_level": level, "zlib_GBps_one_thread": len(sample) / deflate_s / 1e9,
            "zlib_ratio": len(packed) / len(sample), "write_fsync_GBps": len(sample) / write_s / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="calls in the timed window of a device call")
    ap.add_argument("--rounds", type=int, default=5, help="rounds in which the compared calls alternate")
    ap.add_argument("--scan-rounds", type=int, default=3, help="timed rounds of each streamed scan, behind a warm one")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd import read_write as rw
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
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
    batches = [fastq_cut_device(ix, t) for t in texts]
    *kept, filter_totals = filter_reads_device(ix, ReadFilter(), *batches)
    torch.cuda.synchronize()
    calls = {"format_call_wide": lambda: rw.format_reads_device(ix, texts, batches, kept, n, gather=rw.WIDE),
             "format_call_bytes": lambda: rw.format_reads_device(ix, texts, batches, kept, n, gather=rw.BYTES),
             "read_filter_call_defaults": lambda: filter_reads_device(ix, ReadFilter(), *batches)}
    if a.trace_only:
        for _ in range(a.steps + 1):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        return
    out = {"tool": "tools/bench_read_write.py", "git_head": commit(),
           "input": {"pairs": n, "read_len": L, "shape": "IDX-D", "touched": "5 pairs in 20",
                     "text_bytes": int(texts[0].numel() + texts[1].numel()), "behind": "the read filter with its defaults"},
           "resource_usage": resource_usage()}
    out["no_kernel_spills"] = all(k.get("scratch_bytes_per_lane") == 0 and k.get("vgpr_spill") == 0
                                  for k in out["resource_usage"].values()) and len(out["resource_usage"]) >= 3
    wide = rw.format_reads_device(ix, texts, batches, kept, n, gather=rw.WIDE)
    plain = rw.format_reads_device(ix, texts, batches, kept, n, gather=rw.BYTES)
    totals = wide[2].cpu().tolist()
    written = totals[2] + totals[3]
    out["totals_of_one_call"] = dict(zip(("records", "bases", "bytes_r1", "bytes_r2", "not_written"), totals))
    out["wide_and_bytes_give_the_same_text"] = all(
        torch.equal(w[:totals[2 + s]], p[:totals[2 + s]]) for s, (w, p) in enumerate(zip(wide[0], plain[0])))
    del wide, plain
    seconds = {name: [] for name in calls}
    for k in range(1 + a.rounds):   # the compared calls alternate; round 0 warms them up
        for name, fn in calls.items():
            s = device_seconds(fn, a.steps)
            if k:
                seconds[name].append(s)
    med = {name: statistics.median(s) for name, s in seconds.items()}
    for name in calls:
        out[name] = {"seconds": med[name], "rounds": seconds[name], "calls_timed": a.steps,
                     "pairs_per_second": n / med[name]}
        if name != "read_filter_call_defaults":
            out[name].update(relative_to_read_filter_call=med[name] / med["read_filter_call_defaults"],
                             bytes_written=written, written_GBps=written / med[name] / 1e9)
    out["format_call_wide"]["relative_to_bytes"] = med["format_call_wide"] / med["format_call_bytes"]
    sample_text = rw.format_reads_device(ix, texts, batches, kept, n)[0][0][:min(totals[2], 64 << 20)].cpu().numpy().tobytes()
    del batches, kept

    pinned = []
    for t in texts:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del texts
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as folder:
        out["host"] = host_throughput(sample_text, 4, folder)
        del sample_text
        ways = {"without_writer": None, "plain_output": ("o1.fq", "o2.fq"), "gz_output": ("o1.fq.gz", "o2.fq.gz")}
        streamed = {name: [] for name in ways}
        results = {}
        for k in range(1 + a.scan_rounds):   # (round 0 warms all three up)
            for name, files in ways.items():
                kw = {}
                if files is not None:
                    kw["write_reads"] = rw.ReadWriter(*[os.path.join(folder, f) for f in files])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hits = chunks = records = 0
                for chunk in scan_pair_source_stream(ix, ArraySource(pinned[0]), ArraySource(pinned[1]),
                                                     a.chunk_mb << 20, max_read_len=None, read_filter=ReadFilter(), **kw):
                    hits += int(chunk[0].shape[0])
                    records += chunk[4].get("written_records", 0)
                    chunks += 1
                spent = time.perf_counter() - t0
                results[name] = {"hit_records": hits, "written_records": records}
                if files is not None:
                    results[name]["file_bytes"] = [os.path.getsize(os.path.join(folder, f)) for f in files]
                if k:
                    streamed[name].append(spent)
        out["streamed_pair_scan"] = {name: dict(results[name], seconds=statistics.median(s), rounds=s)
                                     for name, s in streamed.items()}
        base = out["streamed_pair_scan"]["without_writer"]["seconds"]
        out["streamed_pair_scan"].update(
            chunk_bytes=a.chunk_mb << 20, chunks=chunks,
            plain_over_without=out["streamed_pair_scan"]["plain_output"]["seconds"] / base,
            gz_over_without=out["streamed_pair_scan"]["gz_output"]["seconds"] / base,
            note="all three with the read filter; the files go to a temporary directory of this host, one writer thread "
                 "a file, zlib level 4 in that thread: see host for what one thread deflates and the directory takes")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
