#!/usr/bin/env python3
"""Multi-CSV mode from streamed FASTQ files on one MI355X: one ``scan_multi_csv_report(chunk_bytes=c)`` against what a
user had to do without it, one ``scan_pair_end_report(chunk_bytes=c)`` (or ``scan_single_end_report``) per CSV.

Writes a synthetic PANEL FASTQ pair (synth.make_pairs over an IDX-D gene set, 1 M pairs of 150 bases by default; plain
and gzipped), a FASTA holding a druggable-shaped (IDX-D) and a cancer-shaped (IDX-C) gene set, their two fusion CSVs and
a list of ``--csvs`` entries alternating between them, to a temporary directory.  Then

  (a) ``routes``: per layout, file format and chunk size, ``--runs`` times each and alternating — the K single-CSV
      streamed scans, the one streamed multi-CSV scan, and (for orientation) the resident multi-CSV scan: wall time of
      the whole calls, index builds and host tails included, with a parity flag;
  (b) ``handback``: one chunk of ``--chunk-mb[0]`` MiB scanned against the K indexes, its results handed to the host two
      ways, ``--runs`` times each and alternating — ``pack_scans_device`` + ``download()`` against the K
      ``PairScan.download()`` + ``HitNames.download()`` calls — HIP events and wall time around the hand-back alone;
  (c) the pack kernels' own time is not taken here: run ``--step handback --profile-mode`` of this file under
      ``rocprofv3 --kernel-trace --stats`` in a run of its own (the program after ``--``) and divide the ``gf_pk_k_*``
      rows by (b)'s chunk wall time.

Result (minimum, median, maximum per side) to ``--out``; what was left out of a run says "not measured".  The parent
process never opens the GPU: every step is a child process of this file under its own ``timeout``, and the first one
that fails ends the run."""
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

SHAPES = ("IDX-D", "IDX-C")


def _paths(d):
    return {k: os.path.join(d, v) for k, v in (("fa", "ref.fa"), ("IDX-D", "druggable.csv"), ("IDX-C", "cancer.csv"),
                                               ("lst", "panels.txt"), ("r1", "R1.fq"), ("r2", "R2.fq"),
                                               ("z1", "R1.fq.gz"), ("z2", "R2.fq.gz"))}


def step_files(a):
    """FASTA, the two CSVs, the list, R1 / R2 plain and gzipped (no GPU: the reads are drawn on the host)."""
    from genefuserust_amd import synth
    p = _paths(a.dir)
    sets = {s: synth.make_geneset(s) for s in SHAPES}
    with open(p["fa"], "wb") as fa:
        for shape, genes in sets.items():
            tag = shape[-1]   # (both sets name their genes alike: a contig per set and gene)
            with open(p[shape], "w") as f:
                for name, s, r in zip(genes.names, genes.seqs, genes.reversed_flags):
                    fa.write(b">%s_%s\n%s\n" % (tag.encode(), name.encode(), s))
                    h = len(s) // 2   # two exons; a reversed gene lists them with descending starts (gene.rs:90-105)
                    ex = ((1, h + 1, len(s)), (2, 1, h)) if r else ((1, 1, h), (2, h + 1, len(s)))
                    f.write(">%s,%s_%s:1-%d\n%s\n\n" % (name, tag, name, len(s), "\n".join("%d,%d,%d" % e for e in ex)))
    with open(p["lst"], "w") as f:
        f.write("".join(p[SHAPES[k % 2]] + "\n" for k in range(a.csvs)))
    pr = synth.make_pairs(sets["IDX-D"], a.pairs, read_len=a.read_len, mix="PANEL", seed=20240607, device="cpu")
    off = pr.offsets.numpy()
    for key, zkey, bases, quals, tag in (("r1", "z1", pr.l_bases, pr.l_quals, b"1"), ("r2", "z2", pr.r_bases, pr.r_quals, b"2")):
        b, q = bases.numpy().tobytes(), quals.numpy().tobytes()
        with open(p[key], "wb") as f:
            for i in range(off.shape[0] - 1):
                f.write(b"@SYN:1:FC:1:%d:%d:%d/%s\n%s\n+\n%s\n" % (i // 100000, i % 100000, i, tag, b[off[i]:off[i + 1]],
                                                                     q[off[i]:off[i + 1]]))
        if "gz" in a.formats:
            with open(p[key], "rb") as f, gzip.open(p[zkey], "wb", compresslevel=4) as z:
                shutil.copyfileobj(f, z, 1 << 24)
    print(json.dumps({"pairs": a.pairs, "read_len": a.read_len, "csvs": a.csvs, "shapes": [SHAPES[k % 2] for k in range(a.csvs)],
                      "bytes": {k: os.path.getsize(p[k]) for k in ("r1", "r2", "z1", "z2") if os.path.exists(p[k])}}))


def _summary(xs, unit="s", digits=3):
    return {"min_" + unit: round(min(xs), digits), "median_" + unit: round(statistics.median(xs), digits),
            "max_" + unit: round(max(xs), digits), "runs_" + unit: [round(x, digits) for x in xs]}


def step_routes(a):
    """One layout, one file format, one chunk size: K single-CSV streamed scans, one streamed multi-CSV scan and the
    resident multi-CSV scan, alternating."""
    import torch
    from genefuserust_amd import report_text
    from genefuserust_amd.multi_csv_scan import read_csv_list, scan_multi_csv_report
    from genefuserust_amd.scan import scan_pair_end_report, scan_single_end_report
    p = _paths(a.dir)
    r1, r2 = (p["z1"], p["z2"]) if a.zipped else (p["r1"], p["r2"])
    reads = (r1, r2) if a.layout == "paired" else (r1,)
    c = a.chunk_mb[0] << 20
    csvs = read_csv_list(p["lst"])

    def per_csv():
        one = scan_pair_end_report if a.layout == "paired" else scan_single_end_report
        return [(csv, *one(p["fa"], csv, *reads, chunk_bytes=c)) for csv in csvs]
    sides = {"k_single_csv_streamed": per_csv,
             "multi_csv_streamed": lambda: scan_multi_csv_report(p["fa"], p["lst"], *reads, chunk_bytes=c),
             "multi_csv_resident": lambda: scan_multi_csv_report(p["fa"], p["lst"], *reads)}

    def run(fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    run(sides["multi_csv_streamed"])   # warm: the first call of a process loads the code objects
    times, outs = {k: [] for k in sides}, {}
    for _ in range(a.runs):
        for k, fn in sides.items():
            t, outs[k] = run(fn)
            times[k].append(t)
            print("%s %s: %.3f s" % (a.layout, k, t), file=sys.stderr, flush=True)

    def entries(got, chunks=True):
        return [(csv, report_text(res), {k: v for k, v in cnt.items() if chunks or k != "chunks"}) for csv, res, cnt in got]
    base, multi = times["k_single_csv_streamed"], times["multi_csv_streamed"]
    line = {"layout": a.layout, "zipped": bool(a.zipped), "chunk_mib": a.chunk_mb[0], "csvs": len(csvs),
            **{k: _summary(v) for k, v in times.items()},
            "parity_with_k_single_csv": entries(outs["multi_csv_streamed"]) == entries(outs["k_single_csv_streamed"]),
            "parity_with_resident": entries(outs["multi_csv_streamed"], False) == entries(outs["multi_csv_resident"], False),
            "chunks": outs["multi_csv_streamed"][0][2]["chunks"],
            "baseline_spread_s": round(max(base) - min(base), 3),
            "median_gain_s": round(statistics.median(base) - statistics.median(multi), 3),
            # faster by more than the baseline's own run-to-run spread: its slowest run beats the baseline's fastest
            "multi_faster_beyond_baseline_spread": max(multi) < min(base) and
            statistics.median(base) - statistics.median(multi) > max(base) - min(base),
            "counters_first_entry": outs["multi_csv_streamed"][0][2]}
    print(json.dumps(line))


def step_handback(a):
    """One chunk against K indexes; the hand-back of its K results, packed against buffer by buffer."""
    import numpy as np
    import torch
    from contextlib import ExitStack
    from genefuserust_amd import scan_pack
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.hit_names import hit_names_device
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device, read_csv_list, scan_prepared_pairs_device
    from genefuserust_amd.scan import open_index, read_contigs
    p = _paths(a.dir)
    nbytes = a.chunk_mb[0] << 20
    with ExitStack() as stack:
        contigs = read_contigs(p["fa"])
        by_csv = {csv: stack.enter_context(open_index(contigs, csv))[0] for csv in (p[s] for s in SHAPES)}
        ixs = [by_csv[csv] for csv in read_csv_list(p["lst"])]   # (two indexes serve the K entries: a scan does not care)
        texts = []
        for k in ("r1", "r2"):
            with open(p[k], "rb") as f:
                t = f.read(nbytes)
            texts.append(torch.from_numpy(np.frombuffer(t[:t.rfind(b"\n@") + 1], dtype=np.uint8).copy()).cuda())
        l, r = (fastq_cut_device(ixs[0], t) for t in texts)
        m = min(l.n_records, r.n_records)
        lo, ro = l.offsets[:m + 1], r.offsets[:m + 1]
        nl, nr = int(lo[-1].item()), int(ro[-1].item())
        prepared = prepare_pairs_device(ixs[0], l.bases[:nl], l.quals[:nl], lo, r.bases[:nr], r.quals[:nr], ro, a.read_len)
        scans = [scan_prepared_pairs_device(ix, prepared) for ix in ixs]
        names = [hit_names_device(ix, s, texts[0], l, texts[1], r) for ix, s in zip(ixs, scans)]
        torch.cuda.synchronize()

        def packed():
            return scan_pack.pack_scans_device(scans, names).download()

        def one_by_one():
            return [(s.download(), n.download()) for s, n in zip(scans, names)]
        if a.profile_mode:   # (for rocprofv3: warm, then one hand-back of each kind)
            packed(), one_by_one(), packed(), one_by_one()
            torch.cuda.synchronize()
            print(json.dumps({"profile_mode": True, "pairs_in_chunk": m}))
            return
        got, want = packed(), one_by_one()
        same = all(u.rec.tobytes() == w[0][0].tobytes() and u.bases == w[0][1] and u.quals == w[0][2] and u.names == w[1]
                   and u.bits == 0 for u, w in zip(got, want))
        sides = {"packed": packed, "k_downloads": one_by_one}
        wall, dev = {k: [] for k in sides}, {k: [] for k in sides}
        for _ in range(a.runs):
            for k, fn in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                wall[k].append((time.perf_counter() - t0) * 1e3)
                dev[k].append(e0.elapsed_time(e1))
        spread = max(wall["k_downloads"]) - min(wall["k_downloads"])
        line = {"chunk_mib": a.chunk_mb[0], "pairs_in_chunk": m, "csvs": len(ixs),
                "hits_per_scan": [int(u.totals["hits"]) for u in got], "same_results": same,
                "wall": {k: _summary(v, "ms", 4) for k, v in wall.items()},
                "hip_events": {k: _summary(v, "ms", 4) for k, v in dev.items()},
                "k_downloads_spread_ms": round(spread, 4),
                "packed_faster_beyond_that_spread": max(wall["packed"]) < min(wall["k_downloads"]) and
                statistics.median(wall["k_downloads"]) - statistics.median(wall["packed"]) > spread}
        print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--csvs", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk-mb", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--layouts", nargs="+", default=["paired", "single"], choices=["paired", "single"])
    ap.add_argument("--formats", nargs="+", default=["plain", "gz"], choices=["plain", "gz"])
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_csv_stream_bench.json"))
    ap.add_argument("--step", choices=["files", "routes", "handback"], help="(internal) run one step in this process")
    ap.add_argument("--dir")
    ap.add_argument("--layout", choices=["paired", "single"])
    ap.add_argument("--zipped", type=int, default=0)
    ap.add_argument("--profile-mode", action="store_true", help="with --step handback: warm, one hand-back of each kind")
    a = ap.parse_args()
    if a.step:
        {"files": step_files, "routes": step_routes, "handback": step_handback}[a.step](a)
        return
    common = ["--pairs", str(a.pairs), "--read-len", str(a.read_len), "--csvs", str(a.csvs), "--runs", str(a.runs),
              "--formats"] + a.formats
    result = {"tool": "tools/bench_multi_csv_stream.py", "runs_each": a.runs, "order": "alternating", "a_routes": [],
              "c_pack_kernels_share": "not measured"}
    wanted = [(lay, z, mb) for lay in ("paired", "single") for z in ("plain", "gz") for mb in (16, 64)]
    steps = [("files", ["--chunk-mb", str(a.chunk_mb[0])])]
    for lay, fmt, mb in wanted:
        if lay in a.layouts and fmt in a.formats and mb in a.chunk_mb:
            steps.append(("routes", ["--layout", lay, "--zipped", str(int(fmt == "gz")), "--chunk-mb", str(mb)]))
        else:
            result["a_routes"].append({"layout": lay, "zipped": fmt == "gz", "chunk_mib": mb, "result": "not measured"})
    steps.append(("handback", ["--chunk-mb", str(a.chunk_mb[0])]))
    with tempfile.TemporaryDirectory() as d:
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
                result["a_routes"].append(line)
            else:
                result["b_handback"] = line
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
