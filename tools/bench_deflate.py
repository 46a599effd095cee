#!/usr/bin/env python3
"""The device deflate (genefuserust_amd/deflate.py, libgfdeflate.so) on the 1 M-pair FASTQ pair of
tools/bench_read_filter.py (its generator and its rewrite) behind the read filter with its defaults — the input of
tools/bench_read_write.py.

    the deflate call            against the format call whose output it takes; the compared calls alternate round by
                                round — a warm round, then --rounds rounds of --steps calls — and the median round counts
    the streamed pair scan      with the read filter and .gz output, four ways in turn: without the writer, the host route
                                at zlib levels 1 and 4, and the device route
    bytes                       what the device route writes against zlib at levels 1 and 4 over the same members of
                                65280 bytes, on a sample of the bench text and on FASTQ text with binned qualities in
                                runs (tests/deflate_cases.py)
    --trace-only                the deflate and the format call alone, --steps times each, for a kernel trace in a run
                                of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_deflate.py --trace-only)

One JSON document on stdout and, with --out, in a file (profiles/deflate_bench.json)."""
import argparse
import gzip
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

TEXT = 65280


def resource_usage():
    """VGPRs, LDS and scratch of each gf_df_k_* kernel, from the compiler's remarks (make resource-usage compiles the
    same file with the same flags)."""
    src = os.path.join(ROOT, "genefuserust_amd", "scan_csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "gf_deflate.hip"],
                          cwd=src, capture_output=True, text=True)
    out, name = {}, None
    for line in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"gf_df_k_[a-z]+", m.group(1))
            name = name.group(0) if name else None
            if name:
                out.setdefault(name, {})
        for key, label in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                           ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"), ("vgpr_spill", r"VGPRs Spill: (\d+)")):
            m = re.search(label, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def bytes_against_zlib(text: bytes, device_bytes: int) -> dict:
    """``device_bytes`` (the members of ``text`` as the device wrote them) against zlib over the same members."""
    out = {"text_bytes": len(text), "members": -(-len(text) // TEXT), "device_bytes": device_bytes,
           "device_ratio": device_bytes / len(text)}
    for level in (1, 4):
        t0 = time.perf_counter()
        packed = 0
        for k in range(0, len(text), TEXT):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            packed += len(c.compress(text[k:k + TEXT]) + c.flush()) + 26      # (the BGZF frame around the stream)
        out["zlib_level_%d" % level] = {"bytes": packed, "ratio": packed / len(text), "device_over_zlib": device_bytes / packed,
                                        "GBps_one_thread": len(text) / (time.perf_counter() - t0) / 1e9}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5, help="calls in the timed window of a device call")
    ap.add_argument("--rounds", type=int, default=5, help="rounds in which the compared calls alternate")
    ap.add_argument("--scan-rounds", type=int, default=3, help="timed rounds of each streamed scan, behind a warm one")
    ap.add_argument("--sample-mb", type=int, default=16, help="the text zlib is run on for the byte counts")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd import deflate as df
    from genefuserust_amd import read_write as rw
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    from genefuserust_amd.stream import pinned_empty
    from tests.deflate_cases import binned_fastq_text
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
    out_texts, out_offs, format_totals = rw.format_reads_device(ix, texts, batches, kept, n)
    torch.cuda.synchronize()
    lengths = [off[n:n + 1] for off in out_offs]
    calls = {"deflate_call_both_sides": lambda: [df.deflate_device(t, ln) for t, ln in zip(out_texts, lengths)],
             "format_call": lambda: rw.format_reads_device(ix, texts, batches, kept, n)}
    if a.trace_only:
        for _ in range(a.steps + 1):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        return
    out = {"tool": "tools/bench_deflate.py", "git_head": commit(),
           "input": {"pairs": n, "read_len": L, "shape": "IDX-D", "touched": "5 pairs in 20",
                     "text_bytes": int(texts[0].numel() + texts[1].numel()), "behind": "the read filter with its defaults"},
           "resource_usage": resource_usage()}
    out["no_scratch"] = all(k.get("scratch_bytes_per_lane") == 0 for k in out["resource_usage"].values()) \
        and len(out["resource_usage"]) == 3
    written = [int(x) for x in format_totals.cpu().tolist()[2:4]]
    first = [df.deflate_device(t, ln) for t, ln in zip(out_texts, lengths)]
    totals = [[int(x) for x in d[2].cpu().tolist()] for d in first]
    out["totals_of_one_call"] = [dict(zip(("members", "text_bytes", "compressed_bytes", "stored", "dynamic"), t)) for t in totals]
    assert [t[1] for t in totals] == written
    # the output inflates to the text (the first 64 members of R1, under zlib)
    k = min(64, totals[0][0])
    comp = first[0][0][:int(first[0][1][k].item())].cpu().numpy().tobytes()
    head = gzip.decompress(comp)
    out["output_inflates_to_the_text"] = head == out_texts[0][:min(k * TEXT, written[0])].cpu().numpy().tobytes()
    sample = out_texts[0][:min(written[0], a.sample_mb << 20) // TEXT * TEXT].cpu().numpy().tobytes()
    sample_members = len(sample) // TEXT
    sample_device = int(first[0][1][sample_members].item())
    out["bytes"] = {"bench_text": bytes_against_zlib(sample, sample_device)}
    quals = np.frombuffer(sample[:1 << 20], dtype=np.uint8)
    out["bytes"]["bench_text"]["note"] = ("%d distinct byte values in the first MiB of the text: the generator's qualities "
                                          "are 'F' but for the touched pairs, so this ratio says little about real "
                                          "files; see binned_text" % len(np.unique(quals)))
    binned = binned_fastq_text(a.sample_mb << 20)
    d_binned = torch.from_numpy(np.frombuffer(binned, dtype=np.uint8).copy()).to(dev)
    out["bytes"]["binned_text"] = bytes_against_zlib(binned, int(df.deflate_device(d_binned)[2].cpu().tolist()[2]))
    del first, comp, sample, binned, d_binned
    seconds = {name: [] for name in calls}
    for k in range(1 + a.rounds):   # the compared calls alternate; round 0 warms them up
        for name, fn in calls.items():
            s = device_seconds(fn, a.steps)
            if k:
                seconds[name].append(s)
    med = {name: statistics.median(s) for name, s in seconds.items()}
    for name in calls:
        out[name] = {"seconds": med[name], "rounds": seconds[name], "calls_timed": a.steps,
                     "text_GBps": sum(written) / med[name] / 1e9}
    out["deflate_call_both_sides"]["relative_to_format_call"] = med["deflate_call_both_sides"] / med["format_call"]
    del batches, kept, out_texts, out_offs, lengths

    pinned = []
    for t in texts:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del texts
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as folder:
        ways = {"without_writer": None, "host_level_1": dict(compress_level=1), "host_level_4": dict(compress_level=4),
                "device": dict(deflate="device")}
        streamed = {name: [] for name in ways}
        results = {}
        for k in range(1 + a.scan_rounds):   # (round 0 warms all four up)
            for name, how in ways.items():
                kw = {}
                files = [os.path.join(folder, name + f) for f in ("_1.fq.gz", "_2.fq.gz")]
                if how is not None:
                    kw["write_reads"] = rw.ReadWriter(*files, **how)
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
                if how is not None:
                    results[name]["file_bytes"] = [os.path.getsize(f) for f in files]
                if k:
                    streamed[name].append(spent)
        out["streamed_pair_scan"] = {name: dict(results[name], seconds=statistics.median(s), rounds=s)
                                     for name, s in streamed.items()}
        sp = out["streamed_pair_scan"]
        sp.update(chunk_bytes=a.chunk_mb << 20, chunks=chunks,
                  device_over_host_level_1=sp["device"]["seconds"] / sp["host_level_1"]["seconds"],
                  device_over_host_level_4=sp["device"]["seconds"] / sp["host_level_4"]["seconds"],
                  device_over_without=sp["device"]["seconds"] / sp["without_writer"]["seconds"],
                  device_beats_host_level_1=sp["device"]["seconds"] < sp["host_level_1"]["seconds"],
                  note="all four with the read filter; the files go to a temporary directory of this host, one writer "
                       "thread a file; on the host route zlib runs in that thread, on the device route it writes the "
                       "members as they are")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
