#!/usr/bin/env python3
"""The report tail on the host (``tail="host"``) against in bulk (``tail="device"``, libgfreport.so), on one MI355X.

Planted matches as tests/test_fusion_result.py's ``planted_matches`` builds them — 20 GA|GB junctions with equal
numbers of 150-base reads each, 1 % substitutions, breaks jittered by up to two bases — go through the tail of
``scan.finish_matches`` and ``scan.report_matches``: the filters, the sort, the per-gene-pair grouping, the clustering
with the break refinement.  Timed per step and in all, host and device at 8 000 and 32 000 matches with a parity flag,
the device tail alone at 100 000.  Result to ``--out``, with the commit the tree stands on and a hash of the tail's
sources.

The parent process never opens the GPU: every size is a child process of this file under its own ``timeout``, and the
first one that fails ends the run."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(TOOLS, "..")
sys.path.insert(0, ROOT)

CSV = ">GA,chr1:1000-7000\n1,1000,3000\n2,4000,7000\n\n>GB,chr2:500-6500\n1,500,2500\n2,3500,6500\n"
JUNCTIONS, READ_LEN = 20, 150
SOURCES = ("genefuserust_amd/report_tail.py", "genefuserust_amd/fusion_result.py", "genefuserust_amd/scan_csrc/gf_rp_core.h",
           "genefuserust_amd/scan_csrc/gf_rp_kernels.h", "genefuserust_amd/scan_csrc/gf_report.hip")


def planted(n_matches, seed=1):
    import numpy as np
    from genefuserust_amd import Fusion, GenePos, ReadMatch
    from genefuserust_amd.fusion_result import get_ref_seq
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = [acgt[rng.integers(0, 4, size=6000)].tobytes() for _ in range(2)]
    ms = []
    for j in range(JUNCTIONS):
        lp, rp = 400 + 250 * j, 600 + 250 * j
        for k in range(n_matches // JUNCTIONS):
            a = int(rng.integers(30, READ_LEN - 29))
            seq = bytearray(get_ref_seq(seqs[0], lp - a + 1, lp) + get_ref_seq(seqs[1], rp, rp + READ_LEN - a - 1))
            for i in np.nonzero(rng.random(READ_LEN) < 0.01)[0]:
                seq[i] = b"ACGT"[(b"ACGT".index(seq[i]) + 1 + int(rng.integers(0, 3))) % 4]
            jit = int(rng.integers(-2, 3))
            gap = 0 if (k % 4 == 0 and jit == 0) else int(rng.integers(1, 3))
            ms.append(ReadMatch(bytes(seq), a - 1 + jit, GenePos(0, lp + jit), GenePos(1, rp + jit), gap, 0, 0, bool(k & 1),
                                b"@read%06d_%d/1" % (k, j), m_quality=b"F" * READ_LEN))
    order = rng.permutation(len(ms))
    return [ms[i] for i in order], Fusion.parse_csv_text(CSV), [s.decode() for s in seqs]


def run_tail(tail, ms, fusions, fseq, mapper_filter, device):
    """(results, counters, seconds per step) of one tail over ``ms``."""
    from genefuserust_amd import report_tail
    from genefuserust_amd.fusion_mapper import FusionMapper
    from genefuserust_amd.fusion_result import Settings, cluster_matches, group_and_sort
    t = [time.perf_counter()]
    if tail == "device":
        kept, removed = report_tail.filter_matches_device(ms, 50, device)
        t.append(time.perf_counter())
        groups = group_and_sort(report_tail.order_matches(kept), len(fusions), report_tail.order_matches)
        t.append(time.perf_counter())
        results = report_tail.cluster_matches_device(groups, fusions, fseq, Settings(), device)
    else:
        kept, removed = mapper_filter(ms, 50)
        t.append(time.perf_counter())
        groups = group_and_sort(FusionMapper.sort_matches(kept), len(fusions))
        t.append(time.perf_counter())
        results = cluster_matches(groups, fusions, fseq, Settings())
    t.append(time.perf_counter())
    secs = dict(filter_s=round(t[1] - t[0], 4), sort_and_group_s=round(t[2] - t[1], 4), cluster_s=round(t[3] - t[2], 4),
                total_s=round(t[3] - t[0], 4))
    return results, removed, secs


def step_size(a):
    import torch
    from genefuserust_amd.fusion_mapper import FusionMapper
    from genefuserust_amd.fusion_result import report_json
    assert torch.cuda.is_available(), "the device tail needs the GPU"
    ms, fusions, fseq = planted(a.matches)
    host_filter = object.__new__(FusionMapper).filter_matches   # (filter_matches reads nothing of the mapper)
    run_tail("device", ms[:200], fusions, fseq, host_filter, 0)             # (warm: library and code objects loaded)
    row = {"matches": len(ms)}
    got, removed, row["device"] = run_tail("device", ms, fusions, fseq, host_filter, 0)
    row["kept"] = len(ms) - sum(removed.values())
    row["fusions"] = len(got)
    if a.host:
        want, removed_h, row["host"] = run_tail("host", ms, fusions, fseq, host_filter, 0)
        row["same_results"] = got == want and removed == removed_h and \
            report_json(got, "c", "v", "t") == report_json(want, "c", "v", "t")
        row["host_over_device"] = round(row["host"]["total_s"] / row["device"]["total_s"], 2)
    print(json.dumps(row))


def commit():
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode == 0:
        return head.stdout.strip()
    try:   # (a snapshot without .git: tools/stamp_head.sh wrote the commit before it was taken)
        return json.load(open(os.path.join(ROOT, ".git_head"))).get("git_head")
    except (OSError, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--both", type=int, nargs="*", default=[8000, 32000], help="sizes timed on the host and the device")
    ap.add_argument("--device-only", type=int, nargs="*", default=[100000])
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_tail_bench.json"))
    ap.add_argument("--matches", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--host", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.matches:
        return step_size(a)
    sha = hashlib.sha256()
    for rel in SOURCES:
        sha.update(open(os.path.join(ROOT, rel), "rb").read())
    result = {"config": {"junctions": JUNCTIONS, "read_len": READ_LEN, "deletion_threshold": 50},
              "commit": commit(), "tail_sources_sha256": sha.hexdigest(), "sizes": []}
    for n, host in [(n, True) for n in a.both] + [(n, False) for n in a.device_only]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--matches", str(n)]
        p = subprocess.run(cmd + (["--host"] if host else []), stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("%d matches failed with exit status %d: nothing after it is run" % (n, p.returncode), file=sys.stderr)
            return p.returncode
        result["sizes"].append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(result["sizes"][-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
