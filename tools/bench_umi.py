#!/usr/bin/env python3
"""The UMI calls (genefuserust_amd/umi.py, libgfumi.so) on the 1 M-pair FASTQ pair of tools/bench_read_filter.py (its
generator and its rewrite), with an 8-base UMI and a 2-base spacer in front of both mates for the inline sources, and
Illumina-style names of 67 bytes — '@A00123:45:HXXXXXXXX:1:1101:0000000042:ACGTACGT+ACGTACGT 1:N:0:ACGT' — for the name
source.

    the cut call (per_read, 8 + 2)     against the read filter call with its defaults on the same input; the compared
    the names call                      calls alternate round by round, and the median round counts
    the mix call
    the streamed pair scan             without umi and with it (per_read, 8 + 2), on the text with the inline UMIs
    the model on the host              tests/umi_model.py over the first --model-pairs pairs

One JSON document on stdout and, with --out, in a file (profiles/umi_bench.json)."""
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
from tools.bench_read_filter import L, device_seconds, rewrite  # noqa: E402

UMI_LEN, UMI_SKIP = 8, 2
NAME_HEAD, NAME_TAIL = b"@A00123:45:HXXXXXXXX:1:1101:", b" 1:N:0:ACGT"


def commit():
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode == 0:
        return head.stdout.strip()
    try:   # (a snapshot without .git: tools/stamp_head.sh wrote the commit before it was taken)
        return json.load(open(os.path.join(ROOT, ".git_head"))).get("git_head")
    except (OSError, ValueError):
        return None


def make_umis(n, dev, seed=11):
    """(n, 8) random ACGT per mate; one UMI in 64 holds an N."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8)
    out = []
    for _ in range(2):
        u = acgt[torch.randint(0, 4, (n, UMI_LEN), generator=g)]
        u[torch.arange(0, n, 64), 3] = ord("N")
        out.append(u.to(dev))
    return out


def make_text(bases, quals, umi_pair, n, mate, dev, inline):
    """The FASTQ text of one mate: with ``inline`` the mate's UMI and 'TG' in front of the bases (and ten 'I' in front of
    the qualities) under the name '@r0000000042/1'; without, the bases as they are under the Illumina-style name that
    holds both UMIs."""
    idx = torch.arange(n, device=dev, dtype=torch.int64)
    digits = torch.stack([(48 + (idx // (10 ** (9 - d))) % 10).to(torch.uint8) for d in range(10)], dim=1)
    nl = torch.full((n, 1), 10, dtype=torch.uint8, device=dev)

    def const(b):
        return torch.tensor(list(b), dtype=torch.uint8, device=dev).expand(n, len(b))
    if inline:
        name = [const(b"@r"), digits, const(b"/%d" % mate)]
        seq = [umi_pair[mate - 1], const(b"TG"), bases.view(n, L)]
        qual = [const(b"I" * (UMI_LEN + UMI_SKIP)), quals.view(n, L)]
    else:
        name = [const(NAME_HEAD), digits, const(b":"), umi_pair[0], const(b"+"), umi_pair[1], const(NAME_TAIL)]
        seq, qual = [bases.view(n, L)], [quals.view(n, L)]
    return torch.cat(name + [nl] + seq + [nl, const(b"+"), nl] + qual + [nl], dim=1).reshape(-1)


def resource_usage():
    """VGPRs and scratch of each gf_um_k_* kernel, from the compiler's remarks (make resource-usage compiles the same
    file with the same flags)."""
    src = os.path.join(ROOT, "genefuserust_amd", "scan_csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    done = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", "gf_umi.hip"],
                          cwd=src, capture_output=True, text=True)
    out, name = {}, None
    for line in done.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.search(r"gf_um_k_[a-z_]+", m.group(1))
            name = name.group(0) if name else None
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
    ap.add_argument("--chunk-mb", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="calls in the timed window of a device call")
    ap.add_argument("--rounds", type=int, default=5, help="rounds in which the compared calls alternate")
    ap.add_argument("--model-pairs", type=int, default=20_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd import dedup as dd
    from genefuserust_amd import umi as um
    from genefuserust_amd.chunk_stream import ArraySource
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_filter import ReadFilter, filter_reads_device
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    from genefuserust_amd.stream import pinned_empty
    from tests import umi_model as model
    dev = torch.device("cuda", 0)
    genes = synth.make_geneset("IDX-D")
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    n = a.pairs
    pr = synth.make_pairs(genes, n, read_len=L, seed=20240302, device="cuda")
    rewrite(pr, n)
    umis = make_umis(n, dev)
    sides = ((pr.l_bases, pr.l_quals), (pr.r_bases, pr.r_quals))
    inline = [make_text(b, q, umis, n, mate, dev, True) for mate, (b, q) in enumerate(sides, 1)]
    named = make_text(pr.l_bases, pr.l_quals, umis, n, 1, dev, False)
    del pr
    out = {"tool": "tools/bench_umi.py", "git_head": commit(),
           "input": {"pairs": n, "read_len": L, "shape": "IDX-D", "touched": "5 pairs in 20",
                     "umi": "%d bases and a spacer of %d in front of both mates" % (UMI_LEN, UMI_SKIP),
                     "name_bytes": len(NAME_HEAD) + 10 + 2 + 2 * UMI_LEN + len(NAME_TAIL),
                     "inline_text_bytes": int(inline[0].numel() + inline[1].numel()),
                     "named_text_bytes_r1": int(named.numel())},
           "resource_usage": resource_usage()}
    out["no_kernel_spills"] = all(k.get("scratch_bytes_per_lane") == 0 and k.get("vgpr_spill") == 0
                                  for k in out["resource_usage"].values()) and len(out["resource_usage"]) >= 3
    batches = [fastq_cut_device(ix, t) for t in inline]
    named_batch = fastq_cut_device(ix, named)
    config = um.Umi("per_read", UMI_LEN, UMI_SKIP)
    torch.cuda.synchronize()
    *cut, codes, cut_totals = um.cut_umis_device(ix, config, *batches)
    name_codes, name_totals = um.name_umis_device(ix, named, named_batch)
    rec_keys = dd.keys_device(ix, *cut)
    calls = {"cut_call_per_read_8_2": lambda: um.cut_umis_device(ix, config, *batches),
             "names_call": lambda: um.name_umis_device(ix, named, named_batch),
             "mix_call": lambda: um.mix_keys_device(ix, rec_keys, codes),
             "read_filter_call_defaults": lambda: filter_reads_device(ix, ReadFilter(), *batches)}
    seconds = {name: [] for name in calls}
    for _ in range(a.rounds):   # the compared calls alternate
        for name, fn in calls.items():
            seconds[name].append(device_seconds(fn, a.steps))
    med = {name: statistics.median(s) for name, s in seconds.items()}
    for name in calls:
        out[name] = {"seconds": med[name], "rounds": seconds[name], "calls_timed": a.steps,
                     "pairs_per_second": n / med[name]}
        if name != "read_filter_call_defaults":
            out[name]["relative_to_read_filter_call"] = med[name] / med["read_filter_call_defaults"]
    moved = 2 * int(cut[0].bases.numel() + cut[1].bases.numel())     # bases and qualities, written once
    out["cut_call_per_read_8_2"]["bytes_gathered"] = moved
    out["cut_call_per_read_8_2"]["gathered_bytes_per_second"] = moved / med["cut_call_per_read_8_2"]
    out["totals_of_one_cut"] = dict(zip(("seen", "tagged", "missing", "with_n", "bases_cut", "too_short", "bases_removed"),
                                        cut_totals.cpu().tolist()))
    out["totals_of_one_names_call"] = dict(zip(("seen", "tagged", "missing", "with_n"), name_totals.cpu().tolist()[:4]))
    # (the codes of the two sources differ by construction — a pair's code mixes H(u1) and H(u2), a name's field is one
    #  string — so only the counts agree)
    out["codes_nonzero"] = {"cut": int((codes != 0).sum()), "names": int((name_codes != 0).sum())}
    host = [t.view(n, -1)[:a.model_pairs].cpu().numpy() for t in inline]
    del batches, named_batch, cut, codes, name_codes, rec_keys, named

    t0 = time.perf_counter()
    records = []
    for x, y in zip(*host):
        (xb, xq), (yb, yq) = [(bytes(r[15:15 + L + 10]), bytes(r[18 + L + 10:18 + 2 * (L + 10)])) for r in (x, y)]
        records.append(((xb, xq), (yb, yq)))
    got = model.cut(model.PER_READ, UMI_LEN, UMI_SKIP, records)
    keys = model.dedup_keys(got.records, got.codes)
    out["model_on_the_host"] = {"pairs": len(records), "seconds": time.perf_counter() - t0, "tagged": got.totals[1],
                                "keys": len(set(keys))}

    pinned = []
    for t in inline:
        h = pinned_empty(t.numel(), np.uint8)
        h[:] = t.cpu().numpy()
        pinned.append(h)
    del inline
    torch.cuda.empty_cache()
    streamed = {"without_umi": [], "with_umi": []}
    results = {}
    for k in range(1 + a.rounds):   # (round 0 warms both up)
        for name in streamed:
            kw = {} if name == "without_umi" else {"umi": config}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hits = chunks = tagged = 0
            for chunk in scan_pair_source_stream(ix, ArraySource(pinned[0]), ArraySource(pinned[1]), a.chunk_mb << 20,
                                                 max_read_len=None, **kw):
                hits += int(chunk[0].shape[0])
                tagged += chunk[4].get("umi_reads_tagged", 0)
                chunks += 1
            spent = time.perf_counter() - t0
            results[name] = {"hit_records": hits, "umi_reads_tagged": tagged}
            if k:
                streamed[name].append(spent)
    out["streamed_pair_scan"] = {name: dict(results[name], seconds=statistics.median(s), rounds=s)
                                 for name, s in streamed.items()}
    out["streamed_pair_scan"].update(
        chunk_bytes=a.chunk_mb << 20, chunks=chunks,
        with_over_without=out["streamed_pair_scan"]["with_umi"]["seconds"] /
        out["streamed_pair_scan"]["without_umi"]["seconds"],
        note="without umi the lean cut is scanned, UMI bases included; with it the full cut, the UMI step and the scan "
             "of reads that are 10 bases shorter")
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
