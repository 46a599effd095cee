#!/usr/bin/env python3
"""Single-end reads per second on one MI355X: ONE gf_se_scan_device call (libgfse.so) from records in HBM to the hit
list — the policy of SingleEndScanner::scan_single_end (sescanner.rs:183-205) — against gf_map_reads_device alone on
the same batch, the cost of the empty retry slots, and the file-level scan by both routes (host / device) on a FASTQ
written to a temporary file, with a parity flag.

Synthetic reads per SURVEY.md §8(d): synth.make_reads(mix="PANEL") over an IDX-D gene set (some genes reversed;
half of all reads reverse-complemented, so that junction reads come back in the wrong direction and are retried),
constant qualities.  One JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_frontend import timed  # noqa: E402


def write_fastq(path, bases: bytes, offsets: np.ndarray, qual: int = ord("F")):
    with open(path, "wb") as f:
        for i in range(offsets.shape[0] - 1):
            s = bases[offsets[i]:offsets[i + 1]]
            f.write(b"@r%d/1\n%s\n+\n%s\n" % (i, s, bytes([qual]) * len(s)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--shape", default="IDX-D")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--file-reads", type=int, default=1_000_000, help="reads of the FASTQ of the file-level routes (0: skip)")
    ap.add_argument("--profile-mode", action="store_true", help="one warm scan only (for rocprofv3)")
    a = ap.parse_args()
    from genefuserust_amd import FusionMapper, Indexer, synth
    from genefuserust_amd.read_pair import finish_pair_hits
    from genefuserust_amd.scan import scan_single_end_files
    from genefuserust_amd.single_end import lib as se_lib, scan_single_device
    dev = torch.device("cuda", 0)
    genes = synth.make_geneset(a.shape)
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    n, L = a.reads, a.read_len
    rb = synth.make_reads(genes, n, read_len=L, mix="PANEL", seed=20240505, device="cuda")
    bases, offsets = rb.bases, rb.offsets
    quals = torch.full_like(bases, ord("F"))
    del rb
    torch.cuda.synchronize()
    caps = dict(hits_cap=max(1024, n // 16), bytes_cap=max(1024, n // 16) * L)
    scan = lambda **kw: scan_single_device(ix, bases, quals, offsets, L, check_lengths=False, **caps, **kw)  # noqa: E731
    if a.profile_mode:
        for _ in range(2):
            res = scan()
        torch.cuda.synchronize()
        print(json.dumps({"totals": res.download()[3]}))
        return
    ms_scan, res = timed(scan, a.steps, a.warmup)
    rec, hb, hq, tot = res.download()
    assert tot["overflow"] == 0 and int(res.totals[5].item()) == 0, tot
    counts = torch.empty(n, dtype=torch.uint8, device=dev)
    matches = torch.empty((n, 2, 16), dtype=torch.uint8, device=dev)
    from genefuserust_amd import _lib
    G = _lib.lib()
    st = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    ms_map, _ = timed(lambda: _lib.check(G.gf_map_reads_device(ix._handle(), bases.data_ptr(), offsets.data_ptr(), n, L,
                                                               counts.data_ptr(), matches.data_ptr(), st())),
                      a.steps, a.warmup)
    # the retry pass maps every slot (the number of retries is on the device): what the empty slots cost
    R = int(se_lib().gf_se_retry_capacity(n))
    e_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    e_bases = torch.zeros(64, dtype=torch.uint8, device=dev)
    rc_counts = torch.empty(R, dtype=torch.uint8, device=dev)
    rc_matches = torch.empty((R, 2, 16), dtype=torch.uint8, device=dev)
    ms_empty, _ = timed(lambda: _lib.check(G.gf_map_reads_device(ix._handle(), e_bases.data_ptr() + 16, e_off.data_ptr(), R,
                                                                 L, rc_counts.data_ptr(), rc_matches.data_ptr(), st())),
                        a.steps, a.warmup)
    # ... and inside the scan, where the real retries sit in front of them: the scan at other retry capacities
    sweep = {}
    for cap in (max(1, 2 * tot["retried_reads"]), n // 256, n // 64, n // 16):
        if cap >= max(1, tot["retried_reads"]):
            sweep[str(cap)] = round(timed(lambda: scan(retry_cap=cap), a.steps, a.warmup)[0], 4)
    # a check of the hit list against the host policy on the first reads
    mapper = FusionMapper(ix)
    k_chk = min(n, 20000)
    hb_all = bases[:k_chk * L].cpu().numpy().tobytes()
    reads = [hb_all[i * L:(i + 1) * L] for i in range(k_chk)]
    want = [(i, m.m_read, m.m_read_break, m.m_reversed) for i, m in enumerate(mapper.scan_single_end(reads)) if m is not None]
    got = [(i, m.m_read, m.m_read_break, m.m_reversed) for i, m in finish_pair_hits(mapper, rec, hb, hq) if i < k_chk]
    line = {
        "reads": n, "read_len": L, "shape": a.shape, "mix": "PANEL",
        "se_scan_ms": round(ms_scan, 4), "se_reads_per_s": n / (ms_scan * 1e-3),
        "map_reads_device_ms": round(ms_map, 4), "scan_over_map": round(ms_scan / ms_map, 4),
        "retried_fraction": tot["retried_reads"] / max(n, 1), "hits": tot["hits"],
        "retry_slots": R, "empty_retry_slots_ms": round(ms_empty, 4),
        "se_scan_ms_by_retry_cap": sweep,
        "host_check_reads": k_chk, "host_check_ok": got == want,
    }
    if a.file_reads:
        m = min(a.file_reads, n)
        off = offsets[:m + 1].cpu().numpy()
        text = bases[:int(off[-1])].cpu().numpy().tobytes()
        with tempfile.TemporaryDirectory() as d:
            fa, csv, fq = os.path.join(d, "ref.fa"), os.path.join(d, "f.csv"), os.path.join(d, "R1.fq")
            with open(fa, "wb") as f:
                for name, s in zip(genes.names, genes.seqs):
                    f.write(b">%s\n%s\n" % (name.encode(), s))
            with open(csv, "w") as f:
                for name, s, r in zip(genes.names, genes.seqs, genes.reversed_flags):
                    h = len(s) // 2   # two exons; a reversed gene lists them with descending starts (gene.rs:90-105)
                    ex = ((1, h + 1, len(s)), (2, 1, h)) if r else ((1, 1, h), (2, h + 1, len(s)))
                    f.write(">%s,%s:1-%d\n%s\n\n" % (name, name, len(s), "\n".join("%d,%d,%d" % e for e in ex)))
            write_fastq(fq, text, off)
            out = {}
            for route in ("host", "device"):
                t0 = time.perf_counter()
                out[route] = scan_single_end_files(fa, csv, fq, route=route)
                line["file_%s_s" % route] = round(time.perf_counter() - t0, 3)
            dc = dict(out["device"][1])
            dc.pop("retried_reads", None)
            line["file_reads"] = m
            line["file_parity"] = out["device"][0] == out["host"][0] and dc == out["host"][1]
            line["file_speedup"] = round(line["file_host_s"] / line["file_device_s"], 2)
    print(json.dumps(line))
    ix.close()


if __name__ == "__main__":
    main()
