#!/usr/bin/env python3
"""BGZF inputs of the streamed routes, inflated on the host (``inflate="host"``) against on the device
(``inflate="device"``, libgfinflate.so), on one MI355X.

Writes the 1 M-pair PANEL FASTQ pair of tools/bench_stream_files.py and the FASTA of tools/bench_ref_cut.py to a
temporary directory, each also as BGZF (zlib level 6, members of 65 280 bytes of text, the end-of-file marker), and
times, alternating and ``--runs`` times each, at ``--chunk-mb`` chunks:

  * the streamed pair scan (``scan.scan_pair_end_files``) of the BGZF pair with ``inflate="host"`` and ``"device"``;
  * the reference cut (``ref_cut.cut_gene_slices``) of the BGZF FASTA with both;

wall time of the whole call, minimum and maximum, with a parity flag.  The host route on the same files in the same run
is the baseline, and its own spread the margin.  Also the bare host ``readinto`` loop over the BGZF files (the host's
zlib alone), and ``gf_if_inflate_device`` on one chunk of each file between HIP events, in GB/s of text.  Result to
``--out``.

The file and byte-source steps need no GPU.  The parent process never opens the GPU: every step is a child process of
this file under its own ``timeout``, and the first one that fails ends the run."""
import argparse
import gzip
import json
import multiprocessing
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time
import zlib

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(TOOLS, "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, TOOLS)

MEMBER_TEXT = 65280
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _member(text: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = c.compress(text) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(payload) + 25) + payload
            + struct.pack("<II", zlib.crc32(text), len(text)))


def _slab(text: bytes) -> bytes:
    return b"".join(_member(text[k:k + MEMBER_TEXT]) for k in range(0, len(text), MEMBER_TEXT))


def write_bgzf(src: str, dst: str, pool) -> None:
    """``src`` as BGZF: slabs of 256 members compressed side by side, written in order."""
    slab = 256 * MEMBER_TEXT

    def slabs():
        with open(src, "rb") as f:
            while True:
                b = f.read(slab)
                if not b:
                    return
                yield b
    with open(dst, "wb") as out:
        for z in pool.imap(_slab, slabs()):
            out.write(z)
        out.write(EOF_MARKER)


def _paths(d):
    import bench_ref_cut
    import bench_stream_files
    p = bench_stream_files._paths(d)
    p["ref"], p["ref_gz"] = bench_ref_cut._paths(os.path.join(d, "ref_cut"))   # (both tools call their FASTA ref.fa)
    for k, src in (("b1", "r1"), ("b2", "r2"), ("bref", "ref")):
        p[k] = p[src].replace(".fq", ".bgzf.fq").replace(".fa", ".bgzf.fa") + ".gz"
    return p


def step_files(a):
    import bench_ref_cut
    import bench_stream_files
    bench_stream_files.step_files(a)
    os.makedirs(os.path.join(a.dir, "ref_cut"), exist_ok=True)
    bench_ref_cut.step_files(argparse.Namespace(dir=os.path.join(a.dir, "ref_cut"), contig_len=a.contig_len))
    p = _paths(a.dir)
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        for k, src in (("b1", "r1"), ("b2", "r2"), ("bref", "ref")):
            write_bgzf(p[src], p[k], pool)
    print(json.dumps({"member_text_bytes": MEMBER_TEXT, "zlib_level": 6,
                      "bytes": {k: os.path.getsize(p[k]) for k in ("r1", "r2", "ref", "b1", "b2", "bref")}}))


def _span(xs):
    return {"min_s": round(min(xs), 4), "max_s": round(max(xs), 4), "runs": len(xs)}


def _timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def step_source(a):
    """The host's zlib alone: a bare ``readinto`` loop through ``gzip.open`` over each BGZF file."""
    from genefuserust_amd.fastq import FastqByteStream
    p = _paths(a.dir)
    out = {}
    buf = memoryview(bytearray(16 << 20))
    for key in ("b1", "b2", "bref"):
        times, total = [], 0
        for _ in range(a.runs):
            with FastqByteStream(p[key], True) as s:
                t, total = time.perf_counter(), 0
                while True:
                    n = s.readinto(buf)
                    if not n:
                        break
                    total += n
                times.append(time.perf_counter() - t)
        out[key] = dict(_span(times), text_bytes=total, gb_per_s_best=round(total / min(times) / 1e9, 3))
    print(json.dumps(out))


def step_routes(a):
    """The streamed pair scan and the reference cut, ``inflate="host"`` against ``"device"``, alternating (GPU)."""
    import torch
    import bench_ref_cut
    from genefuserust_amd.ref_cut import cut_gene_slices
    from genefuserust_amd.scan import scan_pair_end_files
    assert torch.cuda.is_available(), "the routes need the GPU"
    p = _paths(a.dir)
    c = a.chunk_mb << 20
    out = {}

    def scan(mode):
        res = scan_pair_end_files(p["fa"], p["csv"], p["b1"], p["b2"], chunk_bytes=c, inflate=mode)
        torch.cuda.synchronize()
        return res
    fus = bench_ref_cut._fusions(a.shape, a.contig_len)
    for name, run, key in (("pair_scan", scan, lambda r: ([(m.m_name, m.m_read, m.m_read_break) for m in r[0]], r[1])),
                           ("ref_cut", lambda mode: cut_gene_slices(p["bref"], [fus], c, inflate=mode), lambda r: r)):
        run("device")   # (warm: the first call of a process loads the code objects)
        times = {"host": [], "device": []}
        same = True
        for _ in range(a.runs):
            want, t = _timed(lambda: run("host"))
            times["host"].append(t)
            got, t = _timed(lambda: run("device"))
            times["device"].append(t)
            same = same and key(got) == key(want)
        row = {k: _span(v) for k, v in times.items()}
        row["same_results"] = same
        row["host_over_device_best"] = round(min(times["host"]) / min(times["device"]), 3)
        # faster only when the device's worst run beats the host's best: the host route's own spread is the margin
        row["device_faster_beyond_host_spread"] = max(times["device"]) < min(times["host"])
        if name == "pair_scan":
            row["counters"] = want[1]
        out[name] = row
    print(json.dumps(out))


def step_kernel(a):
    """gf_if_inflate_device on one chunk of each BGZF file between HIP events (GPU)."""
    import numpy as np
    import torch
    from genefuserust_amd import bgzf
    assert torch.cuda.is_available(), "the device call needs the GPU"
    p = _paths(a.dir)
    out = {}
    for key in ("b1", "bref"):
        with open(p[key], "rb") as f:
            comp = np.frombuffer(f.read(a.chunk_mb << 20), dtype=np.uint8)
        w = bgzf.walk_blocks(comp)
        d_comp = torch.from_numpy(comp[:w.comp_bytes].copy()).cuda()
        d_table = torch.from_numpy(w.table.copy()).cuda()
        text = torch.empty(w.text_bytes, dtype=torch.uint8, device="cuda")
        ms = []
        for it in range(a.runs + 2):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            status, totals = bgzf.inflate_device(d_comp, d_table, text)
            e[1].record()
            torch.cuda.synchronize()
            if it >= 2:   # (two warm rounds)
                ms.append(e[0].elapsed_time(e[1]))
        tot = totals.cpu().tolist()
        assert tot == [w.members, -1, 0, w.text_bytes], tot
        with gzip.open(p[key], "rb") as f:
            assert text.cpu().numpy().tobytes() == f.read(w.text_bytes)
        out[key] = {"compressed_bytes": w.comp_bytes, "members": w.members, "text_bytes": w.text_bytes,
                    "ms": [round(min(ms), 3), round(max(ms), 3)],
                    "text_gb_per_s": [round(w.text_bytes / max(ms) / 1e6, 2), round(w.text_bytes / min(ms) / 1e6, 2)]}
    print(json.dumps(out))


STEPS = {"files": step_files, "source": step_source, "routes": step_routes, "kernel": step_kernel}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--shape", default="IDX-D")
    ap.add_argument("--mb", type=int, default=384, help="MiB of FASTA text")
    ap.add_argument("--chunk-mb", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-gpu", action="store_true", help="the steps that need no GPU only")
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_inflate_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help=argparse.SUPPRESS)
    ap.add_argument("--dir", help=argparse.SUPPRESS)
    ap.add_argument("--contig-len", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    import bench_ref_cut
    a.contig_len = (a.mb << 20) * 60 // 61 // len(bench_ref_cut.CONTIGS)
    result = {"config": {"pairs": a.pairs, "read_len": a.read_len, "shape": a.shape, "mb": a.mb, "chunk_mb": a.chunk_mb,
                         "runs": a.runs, "contig_len": a.contig_len}}
    d = tempfile.mkdtemp(prefix="gf_inflate_")
    try:
        for step in ["files", "source"] + ([] if a.no_gpu else ["routes", "kernel"]):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--dir", d, "--contig-len", str(a.contig_len), "--runs", str(a.runs), "--chunk-mb", str(a.chunk_mb),
                   "--pairs", str(a.pairs), "--read-len", str(a.read_len), "--shape", a.shape, "--mb", str(a.mb)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                print("step %s failed with exit status %d: nothing after it is run" % (step, p.returncode), file=sys.stderr)
                return p.returncode
            result[step] = json.loads(p.stdout.strip().splitlines()[-1])
            print(step, json.dumps(result[step]), flush=True)
        if a.no_gpu:
            result["routes"] = result["kernel"] = "not measured"
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
