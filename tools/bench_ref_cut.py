#!/usr/bin/env python3
"""The reference side of a file-level scan: the host reader (``scan.read_contigs`` + ``resolve_gene_slice``) against
the streamed cut on the device (``ref_cut.cut_gene_slices``), on one MI355X.

Writes a synthetic FASTA (contigs named like hg38's, lines of 60 letters, ``--mb`` MiB; plain and gzipped) to a
temporary directory and times, alternating and ``--runs`` times each, the host reader against the cut at the
``--chunk-mb`` sizes, for both index shapes of genefuserust_amd/data/index_shapes.json (the genes' coordinates scaled
into the synthetic contigs, their lengths kept) — wall time of the whole call, with a parity flag.  Also the ceilings
of the byte source: a bare ``readinto`` loop over the plain and the gzipped file (the host's zlib).  And, with HIP
events around single calls on one chunk of that text, gf_rc_index_device and gf_rc_gather_device.  Result (minimum and
maximum of the runs) to ``--out``.

The reader step and the byte-source ceilings need no GPU.  The parent process never opens the GPU: every step is a
child process of this file under its own ``timeout``, and the first one that fails ends the run."""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CONTIGS = ["chr%d" % k for k in range(1, 23)] + ["chrX", "chrY", "chrM"]
HG_LEN = 250_000_000   # the coordinates of the shapes lie below this


def _paths(d):
    return os.path.join(d, "ref.fa"), os.path.join(d, "ref.fa.gz")


def _fusions(shape, contig_len):
    """The shape's genes with their lengths, their starts scaled into contigs of ``contig_len`` bases."""
    from genefuserust_amd.indexer import Fusion, Gene
    shapes = json.load(open(os.path.join(ROOT, "genefuserust_amd", "data", "index_shapes.json")))
    out = []
    for g in shapes[shape]:
        ln = min(g["len"], contig_len // 2)
        start = 1 + int(g["start"] / HG_LEN * (contig_len - ln - 2))
        out.append(Fusion(Gene(g["name"], g["chr"], start, start + ln, g["reversed"])))
    return out


def step_files(a):
    import numpy as np
    fa, gz = _paths(a.dir)
    rng = np.random.default_rng(20240611)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(fa, "wb") as f:
        for name in CONTIGS:
            f.write(b">%s  synthetic contig of %d bases\n" % (name.encode(), a.contig_len))
            seq = letters[rng.integers(0, 4, a.contig_len)]
            full = a.contig_len // 60 * 60
            lines = np.concatenate([seq[:full].reshape(-1, 60), np.full((full // 60, 1), 10, np.uint8)], axis=1)
            f.write(lines.tobytes() + seq[full:].tobytes() + b"\n")
    with open(fa, "rb") as f, gzip.open(gz, "wb", compresslevel=4) as z:
        shutil.copyfileobj(f, z, 1 << 24)
    print(json.dumps({"contigs": len(CONTIGS), "contig_len": a.contig_len,
                      "bytes": {"plain": os.path.getsize(fa), "gz": os.path.getsize(gz)}}))


def _host_reader(path, fusions):
    from genefuserust_amd.indexer import resolve_gene_slice
    from genefuserust_amd.scan import read_contigs
    contigs = read_contigs(path)
    return [resolve_gene_slice(contigs, f.m_gene) for f in fusions]


def _timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t


def _span(xs):
    return {"min_s": round(min(xs), 4), "max_s": round(max(xs), 4), "runs": len(xs)}


def step_source(a):
    """The ceilings of the byte source: a bare ``readinto`` loop over the file, plain and gunzipped."""
    from genefuserust_amd.fastq import FastqByteStream
    out = {}
    buf = memoryview(bytearray(16 << 20))
    for key, path in zip(("plain", "gz"), _paths(a.dir)):
        times, total = [], 0
        for _ in range(a.runs):
            with FastqByteStream(path, key == "gz") as s:
                t, total = time.perf_counter(), 0
                while True:
                    n = s.readinto(buf)
                    if not n:
                        break
                    total += n
                times.append(time.perf_counter() - t)
        out[key] = dict(_span(times), text_bytes=total, gb_per_s_best=round(total / min(times) / 1e9, 3))
    print(json.dumps(out))


def step_reader(a):
    """The host reader alone (no GPU)."""
    out = {}
    for shape in a.shapes:
        fus = _fusions(shape, a.contig_len)
        for key, path in zip(("plain", "gz"), _paths(a.dir)):
            out["%s/%s" % (shape, key)] = _span([_timed(lambda: _host_reader(path, fus))[1] for _ in range(a.runs)])
    print(json.dumps(out))


def step_cut(a):
    """The host reader against the streamed cut, alternating (GPU)."""
    import torch
    from genefuserust_amd.ref_cut import cut_gene_slices
    assert torch.cuda.is_available(), "the cut needs the GPU"
    out = {}
    for shape in a.shapes:
        fus = _fusions(shape, a.contig_len)
        for key, path in zip(("plain", "gz"), _paths(a.dir)):
            cut_gene_slices(path, [fus], a.chunk_mb[0] << 20)   # (warm)
            times = {"host": []}
            same = True
            for _ in range(a.runs):
                want, t = _timed(lambda: _host_reader(path, fus))
                times["host"].append(t)
                for mb in a.chunk_mb:
                    got, t = _timed(lambda: cut_gene_slices(path, [fus], mb << 20)[0])
                    times.setdefault("cut_%dMiB" % mb, []).append(t)
                    same = same and got == want
            row = {k: _span(v) for k, v in times.items()}
            for mb in a.chunk_mb:
                k = "cut_%dMiB" % mb
                row[k]["host_over_cut_best"] = round(min(times["host"]) / min(times[k]), 3)
            row["same_slices"] = same
            row["slice_bytes"] = sum(len(s) for s in want if s)
            out["%s/%s" % (shape, key)] = row
    print(json.dumps(out))


def step_events(a):
    """HIP events around gf_rc_index_device and gf_rc_gather_device on one chunk of the text (GPU)."""
    import numpy as np
    import torch
    from genefuserust_amd.ref_cut import CutPlan, plan_chunk, ref_gather_device, ref_index_device
    assert torch.cuda.is_available(), "the device calls need the GPU"
    out = {}
    fa = _paths(a.dir)[0]
    for mb in a.chunk_mb:
        with open(fa, "rb") as f:
            text = f.read(mb << 20)
        d = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        for shape in a.shapes:
            ix = ref_index_device(d)
            rec = ix.download()
            n, nbytes, rows, _, _, _ = plan_chunk(CutPlan([_fusions(shape, a.contig_len)]), None, rec, d.numel(), False)
            total = rows[-1][3] + rows[-1][2] - rows[-1][1] if rows else 0
            res = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
            ms = {"index": [], "gather": []}
            for it in range(a.runs + 2):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                ref_index_device(d)
                e[1].record()
                ref_gather_device(d[:nbytes], ix, n, rows, total, out=res)
                e[2].record()
                torch.cuda.synchronize()
                if it >= 2:   # (two warm rounds)
                    ms["index"].append(e[0].elapsed_time(e[1]))
                    ms["gather"].append(e[1].elapsed_time(e[2]))
            out["%s/%dMiB" % (shape, mb)] = {
                "text_bytes": d.numel(), "intervals": len(rows), "gathered_bytes": total,
                "index_ms": [round(min(ms["index"]), 4), round(max(ms["index"]), 4)],
                "gather_ms": [round(min(ms["gather"]), 4), round(max(ms["gather"]), 4)],
                "index_gb_per_s_best": round(d.numel() / max(min(ms["index"]), 1e-6) / 1e6, 1),
                "gather_gb_per_s_best": round(nbytes / max(min(ms["gather"]), 1e-6) / 1e6, 1)}
    print(json.dumps(out))


STEPS = {"files": step_files, "source": step_source, "reader": step_reader, "cut": step_cut, "events": step_events}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mb", type=int, default=384, help="MiB of FASTA text")
    ap.add_argument("--chunk-mb", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--shapes", nargs="+", default=["IDX-D", "IDX-C"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-gpu", action="store_true", help="the steps that need no GPU only")
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_cut_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help=argparse.SUPPRESS)
    ap.add_argument("--dir", help=argparse.SUPPRESS)
    ap.add_argument("--contig-len", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    a.contig_len = (a.mb << 20) * 60 // 61 // len(CONTIGS)
    result = {"config": {"mb": a.mb, "chunk_mb": a.chunk_mb, "shapes": a.shapes, "runs": a.runs,
                         "contig_len": a.contig_len}}
    d = tempfile.mkdtemp(prefix="gf_ref_cut_")
    try:
        for step in ["files", "source", "reader"] + ([] if a.no_gpu else ["cut", "events"]):
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--dir", d, "--contig-len", str(a.contig_len), "--runs", str(a.runs), "--chunk-mb",
                   *map(str, a.chunk_mb), "--shapes", *a.shapes]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                print("step %s failed with exit status %d: nothing after it is run" % (step, p.returncode), file=sys.stderr)
                return p.returncode
            result[step] = json.loads(p.stdout.strip().splitlines()[-1])
            print(step, json.dumps(result[step]), flush=True)
        if a.no_gpu:
            result["cut"] = result["events"] = "not measured"
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
