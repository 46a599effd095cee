#!/usr/bin/env python3
"""The file-level scans, whole-file against streamed (``chunk_bytes``), on one MI355X.

Writes a synthetic PANEL FASTQ pair (synth.make_pairs over an IDX-D gene set, 1 M pairs of 150 bases by default; plain
and gzipped) with its FASTA and fusion CSV to a temporary directory and times, alternating and ``--runs`` times each,
``scan.scan_pair_end_files`` / ``scan_single_end_files`` with ``chunk_bytes=None`` (the whole-file route) against the
streamed route at the ``--chunk-mb`` sizes — wall time of the whole call, index build and host tail included, with a
parity flag.  Also, with HIP events around single calls on one chunk of that text: ``hit_names_device`` next to the
pair scan it follows, and the single-end chunk's FASTQ cut with and without the copy of the quality lines next to its
scan.  Result (medians and ranges) to ``--out``.

``--originals`` instead runs the streamed pair scan of the plain files, at the last ``--chunk-mb`` size, once without
and once with ``originals=True`` (the FASTQ records of the hit records gathered behind every chunk's scan,
``hit_records_device``) and writes both times, the bytes gathered and the commit to
``profiles/hit_records_bench.json``: a number to have, not one that is asserted.

The parent process never opens the GPU: every step is a child process of this file under its own ``timeout``, and the
first one that fails ends the run."""
import argparse
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def _paths(d):
    return {k: os.path.join(d, v) for k, v in (("fa", "ref.fa"), ("csv", "f.csv"), ("r1", "R1.fq"), ("r2", "R2.fq"),
                                               ("z1", "R1.fq.gz"), ("z2", "R2.fq.gz"))}


def step_files(a):
    """FASTA, CSV, R1 / R2 plain and gzipped (no GPU: the reads are drawn on the host)."""
    import numpy as np
    from genefuserust_amd import synth
    p = _paths(a.dir)
    genes = synth.make_geneset(a.shape)
    with open(p["fa"], "wb") as f:
        for name, s in zip(genes.names, genes.seqs):
            f.write(b">%s\n%s\n" % (name.encode(), s))
    with open(p["csv"], "w") as f:
        for name, s, r in zip(genes.names, genes.seqs, genes.reversed_flags):
            h = len(s) // 2   # two exons; a reversed gene lists them with descending starts (gene.rs:90-105)
            ex = ((1, h + 1, len(s)), (2, 1, h)) if r else ((1, 1, h), (2, h + 1, len(s)))
            f.write(">%s,%s:1-%d\n%s\n\n" % (name, name, len(s), "\n".join("%d,%d,%d" % e for e in ex)))
    pr = synth.make_pairs(genes, a.pairs, read_len=a.read_len, mix="PANEL", seed=20240607, device="cpu")
    off = pr.offsets.numpy()
    for key, zkey, bases, quals, tag in (("r1", "z1", pr.l_bases, pr.l_quals, b"1"), ("r2", "z2", pr.r_bases, pr.r_quals, b"2")):
        b, q = bases.numpy().tobytes(), quals.numpy().tobytes()
        with open(p[key], "wb") as f:
            for i in range(off.shape[0] - 1):
                f.write(b"@SYN:1:FC:1:%d:%d:%d/%s\n%s\n+\n%s\n" % (i // 100000, i % 100000, i, tag, b[off[i]:off[i + 1]],
                                                                     q[off[i]:off[i + 1]]))
        with open(p[key], "rb") as f, gzip.open(p[zkey], "wb", compresslevel=4) as z:
            shutil.copyfileobj(f, z, 1 << 24)
    print(json.dumps({"pairs": a.pairs, "read_len": a.read_len, "shape": a.shape,
                      "bytes": {k: os.path.getsize(p[k]) for k in ("r1", "r2", "z1", "z2")}}))


def _summary(xs):
    return {"median_s": round(statistics.median(xs), 3), "min_s": round(min(xs), 3), "max_s": round(max(xs), 3),
            "runs_s": [round(x, 3) for x in xs]}


def step_routes(a):
    """One layout and one file format: whole-file and streamed, alternating."""
    import torch
    from genefuserust_amd.scan import scan_pair_end_files, scan_single_end_files
    p = _paths(a.dir)
    r1, r2 = (p["z1"], p["z2"]) if a.zipped else (p["r1"], p["r2"])

    def run(chunk_bytes):
        t0 = time.perf_counter()
        if a.layout == "paired":
            out = scan_pair_end_files(p["fa"], p["csv"], r1, r2, chunk_bytes=chunk_bytes)
        else:
            out = scan_single_end_files(p["fa"], p["csv"], r1, chunk_bytes=chunk_bytes)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    variants = [None] + [mb << 20 for mb in a.chunk_mb]
    run(variants[-1])   # warm: the first call of a process loads the code objects
    times = {v: [] for v in variants}
    outs = {}
    for _ in range(a.runs):
        for v in variants:
            t, outs[v] = run(v)
            times[v].append(t)
    whole = outs[None]
    line = {"layout": a.layout, "zipped": bool(a.zipped), "whole_file": _summary(times[None]), "streamed": {}}
    for v in variants[1:]:
        cnt = dict(outs[v][1])
        chunks = cnt.pop("chunks")
        same = cnt == whole[1] and [(m.m_name, m.m_read, m.m_read_break) for m in outs[v][0]] == \
            [(m.m_name, m.m_read, m.m_read_break) for m in whole[0]]
        line["streamed"]["%d MiB" % (v >> 20)] = {**_summary(times[v]), "chunks": chunks, "parity": same,
                                                  "median_over_whole_file": round(
                                                      statistics.median(times[v]) / statistics.median(times[None]), 3)}
    line["counters"] = whole[1]
    print(json.dumps(line))


def _events(fn, reps=10, warm=3):
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def step_chunk(a):
    """HIP events around single calls on the first chunk of the plain files: the names call next to the pair scan, and
    the single-end chunk's cut with and without the quality copy next to its scan."""
    import numpy as np
    import torch
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.hit_names import hit_names_device
    from genefuserust_amd.indexer import FastaReader, Fusion, Indexer
    from genefuserust_amd.read_pair import scan_pairs_device
    from genefuserust_amd.single_end import scan_single_device
    p = _paths(a.dir)
    ref = FastaReader(p["fa"], True)
    ref.read_all()
    ix = Indexer(ref.m_all_contigs, Fusion.parse_csv(p["csv"]), -1)
    ix.make_index()
    nbytes = a.chunk_mb[-1] << 20
    texts = []
    for k in ("r1", "r2"):
        with open(p[k], "rb") as f:
            t = f.read(nbytes)
        texts.append(torch.from_numpy(np.frombuffer(t[:t.rfind(b"\n@") + 1], dtype=np.uint8).copy()).cuda())
    lean = [fastq_cut_device(ix, t, lean=True) for t in texts]
    m = min(b.n_records for b in lean)
    L = a.read_len
    lo, ro = lean[0].offsets[:m + 1], lean[1].offsets[:m + 1]
    nb = [int(lo[-1].item()), int(ro[-1].item())]

    def pair_scan():
        return scan_pairs_device(ix, lean[0].bases[:nb[0]], lean[0].quals, lo, lean[1].bases[:nb[1]], lean[1].quals, ro, L,
                                 l_qual_off=lean[0].qual_off[:m], r_qual_off=lean[1].qual_off[:m])
    res = pair_scan()
    tot = res.download()[3]
    line = {"chunk_bytes_per_side": nbytes, "pairs_in_chunk": m, "hits": tot["hits"], "hits_cap": int(res.hits.shape[0]),
            "pair_scan": _events(pair_scan),
            "hit_names": _events(lambda: hit_names_device(ix, res, texts[0], lean[0], texts[1], lean[1]))}
    full = fastq_cut_device(ix, texts[0])
    line["single_end"] = {
        "reads_in_chunk": full.n_records,
        "cut_with_quality_copy": _events(lambda: fastq_cut_device(ix, texts[0])),
        "cut_lean": _events(lambda: fastq_cut_device(ix, texts[0], lean=True)),
        "scan": _events(lambda: scan_single_device(ix, full.bases, full.quals, full.offsets, L, check_lengths=False))}
    print(json.dumps(line))
    ix.close()


def step_originals(a):
    """The streamed pair scan without and with the originals, once each (after a warm run)."""
    import torch
    from genefuserust_amd import hit_names
    from genefuserust_amd.scan import scan_pair_end_files
    p = _paths(a.dir)
    chunk_bytes = a.chunk_mb[-1] << 20
    gathered = []
    gather = hit_names.hit_records_device

    def counting(*args, **kwargs):   # (the totals stay on the device until the runs are over)
        gathered.append(gather(*args, **kwargs))
        return gathered[-1]
    hit_names.hit_records_device = counting

    def run(originals):
        t0 = time.perf_counter()
        out = scan_pair_end_files(p["fa"], p["csv"], p["r1"], p["r2"], chunk_bytes=chunk_bytes, originals=originals)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    run(True)   # warm: the first call of a process loads the code objects
    del gathered[:]
    t_without, without = run(False)
    assert not gathered
    t_with, with_ = run(True)
    totals = [[int(x) for x in g.totals.cpu()] for g in gathered]
    print(json.dumps({"chunk_bytes": chunk_bytes, "chunks": with_[1]["chunks"], "without_originals_s": round(t_without, 3),
                      "with_originals_s": round(t_with, 3), "gather_calls": len(totals),
                      "spans_gathered": sum(t[0] for t in totals), "bytes_gathered": sum(t[1] for t in totals),
                      "matches_kept": len(with_[0]), "parity": without[0] == with_[0] and without[1] == with_[1],
                      "counters": with_[1]}))


def commit():
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    if head.returncode == 0:
        return head.stdout.strip()
    try:   # (a snapshot without .git: tools/stamp_head.sh wrote the commit before it was taken)
        return json.load(open(os.path.join(ROOT, ".git_head"))).get("git_head")
    except (OSError, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--shape", default="IDX-D")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk-mb", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds a step may take")
    ap.add_argument("--out", help="default: profiles/stream_files_bench.json, with --originals "
                    "profiles/hit_records_bench.json")
    ap.add_argument("--originals", action="store_true", help="measure the streamed pair scan with and without the "
                    "gather of the original records, and nothing else")
    ap.add_argument("--step", choices=["files", "routes", "chunk", "originals"],
                    help="(internal) run one step in this process")
    ap.add_argument("--dir")
    ap.add_argument("--layout", choices=["paired", "single"])
    ap.add_argument("--zipped", type=int, default=0)
    a = ap.parse_args()
    if a.step:
        {"files": step_files, "routes": step_routes, "chunk": step_chunk, "originals": step_originals}[a.step](a)
        return
    out = a.out or os.path.join(ROOT, "profiles", "hit_records_bench.json" if a.originals else "stream_files_bench.json")
    common = ["--pairs", str(a.pairs), "--read-len", str(a.read_len), "--shape", a.shape, "--runs", str(a.runs),
              "--chunk-mb"] + [str(x) for x in a.chunk_mb]
    if a.originals:
        result = {"tool": "tools/bench_stream_files.py --originals", "commit": commit(), "runs_each": 1}
    else:
        result = {"tool": "tools/bench_stream_files.py", "runs_each": a.runs, "order": "alternating", "routes": []}
    with tempfile.TemporaryDirectory() as d:
        steps = [("files", [])] + [("routes", ["--layout", lay, "--zipped", str(z)])
                                   for lay in ("paired", "single") for z in (0, 1)] + [("chunk", [])]
        if a.originals:
            steps = [("files", []), ("originals", [])]
        for name, extra in steps:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
                   "--dir", d] + common + extra
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:   # a step that failed or ran out of time ends the run: nothing more is started
                print("step %s %s ended with status %d" % (name, extra, r.returncode), file=sys.stderr)
                sys.exit(r.returncode)
            line = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(line), flush=True)
            if name == "files":
                result["input"] = line
            elif name == "routes":
                result["routes"].append(line)
            elif name == "originals":
                result["streamed_pair_scan"] = line
            else:
                result["chunk_calls"] = line
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
