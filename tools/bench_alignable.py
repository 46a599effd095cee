#!/usr/bin/env python3
"""The whole-genome alignable filter on one MI355X (``alignable.alignable_reads_device``) against the only whole-genome
pass there was before it: the reference's ``remove_alignables`` as it is (matcher.py), which scans the same reference
and removes nothing.

The reference is the synthetic genome of tools/bench_ref_cut.py (25 contigs named like hg38's, ``--mb`` MiB of FASTA
text, the same seed and bases), held in memory, with the genes of synth's 30 %-repeat gene set (``make_geneset(
"IDX-D", repeat_frac=0.3)``: 300-base elements of a 20-element family, each some hundred times in the genome) written
over stretches of it.  Two kinds of candidate batches of ``--reads`` reads of 150 bases, 90 % junction reads (75 + 75
bases of two genes) and 10 % whole copies with 0 .. 2 substitutions:

    panel     from the IDX-D panel genes, which are slices of the random contigs
    repeat    from the planted 30 %-repeat genes

Per batch and number of reads: the filter sizes of ``--filter-log2`` alternating, ``--runs`` times each — wall seconds
of the whole call (seeds, sort, staging, upload and scan of every piece) and the scan kernels' time from HIP events,
as GB/s of reference text per run and as the median; the flags must not depend on the filter size.  Then, once per
batch, the as-is pass on the host.  Result to ``--out``.

The parent process never opens the GPU: every step is a child process of this file under its own ``timeout``, and the
first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

READ_LEN = 150


def _reference(a):
    """({name: bytes}, panel gene slices, planted repeat genes)"""
    import numpy as np
    from genefuserust_amd.indexer import resolve_gene_slice
    from genefuserust_amd.synth import make_geneset
    from tools.bench_ref_cut import CONTIGS, _fusions
    contig_len = (a.mb << 20) * 60 // 61 // len(CONTIGS)
    rng = np.random.default_rng(20240611)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    contigs = {name: letters[rng.integers(0, 4, contig_len)] for name in CONTIGS}
    repeat = [np.frombuffer(s, dtype=np.uint8) for s in make_geneset("IDX-D", repeat_frac=0.3).seqs]
    fusions = _fusions("IDX-D", contig_len)
    taken = {name: sorted((f.m_gene.m_start - 1, f.m_gene.m_end) for f in fusions if f.m_gene.m_chr == name)
             for name in CONTIGS}
    at = {name: 0 for name in CONTIGS}
    for k, g in enumerate(repeat):   # (each gene in the next stretch of its contig that holds no panel gene)
        name = CONTIGS[k % len(CONTIGS)]
        p = at[name]
        for s, e in taken[name]:
            if p + g.size + 1000 > s and p < e + 1000:
                p = e + 1000
        assert p + g.size < contig_len, "the repeat genes do not fit: a larger --mb"
        contigs[name][p:p + g.size] = g
        at[name] = p + g.size + 1000
    reference = {name: c.tobytes() for name, c in contigs.items()}
    panel = [resolve_gene_slice(reference, f.m_gene) for f in fusions]
    return reference, panel, [g.tobytes() for g in repeat]


def _reads(genes, n, seed):
    """n reads of READ_LEN bases: 90 % junctions of two genes, 10 % whole copies with 0 .. 2 substitutions."""
    import numpy as np
    rng = np.random.default_rng(seed)
    genes = [g for g in genes if len(g) > 2 * READ_LEN]
    half = READ_LEN // 2
    out = []
    for k in range(n):
        ga, gb = (genes[int(i)] for i in rng.integers(0, len(genes), 2))
        if k % 10:
            p, q = int(rng.integers(0, len(ga) - half)), int(rng.integers(0, len(gb) - READ_LEN + half))
            out.append(ga[p:p + half] + gb[q:q + READ_LEN - half])
        else:
            p = int(rng.integers(0, len(ga) - READ_LEN))
            r = bytearray(ga[p:p + READ_LEN])
            for i in rng.integers(0, READ_LEN, int(rng.integers(0, 3))).tolist():
                r[i] = b"ACGT"[(b"ACGT".find(r[i]) + 1) % 4]
            out.append(bytes(r))
    return out


def _batches(a, panel, repeat):
    return [("%s/%d" % (kind, n), _reads(genes, n, 7 + n)) for kind, genes in (("panel", panel), ("repeat", repeat))
            for n in a.reads]


def step_device(a):
    import numpy as np
    import torch
    from genefuserust_amd.alignable import FILTER_LOG2_DEFAULT, alignable_reads_device
    assert torch.cuda.is_available(), "the filter needs the GPU"
    reference, panel, repeat = _reference(a)
    text_bases = sum(len(c) for c in reference.values())
    out = {"reference_bases": text_bases, "filter_log2_default": FILTER_LOG2_DEFAULT, "batches": {}}
    alignable_reads_device(reference, [panel[0][:READ_LEN]], batch_bytes=a.batch_mb << 20)   # (warm)
    for name, reads in _batches(a, panel, repeat):
        rows = {b: {"wall_s": [], "scan_ms": [], "scan_gb_per_s": []} for b in a.filter_log2}
        flags = None
        for _ in range(a.runs):
            for b in a.filter_log2:   # (alternating)
                stats = {}
                torch.cuda.synchronize()
                t = time.perf_counter()
                got = alignable_reads_device(reference, reads, batch_bytes=a.batch_mb << 20, filter_log2_bits=b, stats=stats)
                rows[b]["wall_s"].append(round(time.perf_counter() - t, 4))
                ms = sum(stats["scan_ms"])
                rows[b]["scan_ms"].append(round(ms, 3))
                rows[b]["scan_gb_per_s"].append(round(stats["text_bytes"] / max(ms, 1e-6) / 1e6, 1))
                rows[b].update(pieces=stats["pieces"], text_bytes=stats["text_bytes"], seeds=stats["seeds"])
                assert flags is None or (got == flags).all(), "the flags depend on the filter size"
                flags = got
        for b in a.filter_log2:
            rows[b]["scan_gb_per_s_median"] = statistics.median(rows[b]["scan_gb_per_s"])
            rows[b]["wall_s_median"] = statistics.median(rows[b]["wall_s"])
        out["batches"][name] = {"reads": len(reads), "alignable": int(np.count_nonzero(flags)),
                                "filter_log2": {str(b): rows[b] for b in a.filter_log2}}
    print(json.dumps(out))


def step_asis(a):
    """The reference's remove_alignables as it is (matcher.py): host code, no GPU."""
    from genefuserust_amd.matcher import Matcher, MatcherPanic
    reference, panel, repeat = _reference(a)
    out = {}
    for name, reads in _batches(a, panel, repeat):
        t = time.perf_counter()
        try:
            m = Matcher(reference, reads)
            removed = sum(m.do_match(r) is not None for r in reads)
            note = None
        except MatcherPanic as e:   # (the reference panics where its inverted test meets a vote)
            removed, note = 0, "MatcherPanic: %s" % e
        out[name] = {"wall_s": round(time.perf_counter() - t, 3), "removed": removed}
        if note:
            out[name]["note"] = note
    print(json.dumps(out))


STEPS = {"device": step_device, "asis": step_asis}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mb", type=int, default=384, help="MiB of FASTA text the reference stands for")
    ap.add_argument("--reads", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--filter-log2", type=int, nargs="+", default=[22, 25, 27, 29, 32])
    ap.add_argument("--batch-mb", type=int, default=256, help="MiB of a piece of reference text")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-gpu", action="store_true", help="the as-is pass only")
    ap.add_argument("--no-asis", action="store_true", help="the device filter only")
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alignable_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    result = {"config": {"mb": a.mb, "reads": a.reads, "read_len": READ_LEN, "filter_log2": a.filter_log2,
                         "batch_mb": a.batch_mb, "runs": a.runs}}
    for step in ([] if a.no_gpu else ["device"]) + ([] if a.no_asis else ["asis"]):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
               "--mb", str(a.mb), "--batch-mb", str(a.batch_mb), "--runs", str(a.runs), "--reads", *map(str, a.reads),
               "--filter-log2", *map(str, a.filter_log2)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("step %s failed with exit status %d: nothing after it is run" % (step, p.returncode), file=sys.stderr)
            return p.returncode
        result[step] = json.loads(p.stdout.strip().splitlines()[-1])
        print(step, json.dumps(result[step]), flush=True)
    for step in ("device", "asis"):
        result.setdefault(step, "not measured")
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
