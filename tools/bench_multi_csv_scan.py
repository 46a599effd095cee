#!/usr/bin/env python3
"""Multi-CSV mode on one MI355X: K fusion CSVs over one resident set of pairs, both ways —

  (a) gf_scan_pairs_device per CSV: merge, stage and scan everything again for every index (the baseline);
  (b) gf_mc_pairs_prepare_device once: merge, gather and pack the pairs (libgfmcsv.so);
  (c) gf_mc_pairs_scan_device per CSV over the prepared pairs;
  (d) the totals for K CSVs: K x (a) against (b) + K x (c);
  (e) the share of pairs that merged.

Synthetic pairs per SURVEY.md §8(d): synth.make_pairs(mix="PANEL") — the pairs of synth.make_pair_reads as R1 / R2
buffers — 150 bases, fragments N(300, 30), cut from an IDX-D gene set; K gene sets alternating between the
druggable-shaped (IDX-D) and the cancer-shaped (IDX-C) index, as the reference's CSV list does.  The indexes are built
outside the timed region.  Times are HIP events on the launch stream around ONE call, after a warm-up; (a) and (c)
alternate within a repeat; median and spread (min, max) over the repeats.  Before timing, every index's result of (c)
is compared with (a)'s, byte for byte.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def one_call_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "repeats": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--csvs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="shrinks the gene sets (rehearsals)")
    ap.add_argument("--profile-mode", action="store_true", help="warm, then one call of each kind (for rocprofv3)")
    a = ap.parse_args()
    from genefuserust_amd import Indexer, synth
    from genefuserust_amd.multi_csv_scan import lib as mc_lib, prepare_pairs_device, scan_prepared_pairs_device
    from genefuserust_amd.read_pair import scan_pairs_device
    n, L, K = a.pairs, a.read_len, a.csvs
    shapes = [("IDX-D", "IDX-C")[k % 2] for k in range(K)]
    sets = {s: synth.make_geneset(s, scale=a.scale) for s in set(shapes)}
    pr = synth.make_pairs(sets["IDX-D"], n, read_len=L, mix="PANEL", seed=20240505, device="cuda")
    t = (pr.l_bases, pr.l_quals, pr.offsets, pr.r_bases, pr.r_quals, pr.offsets)
    # two indexes serve the K list entries: the scan does not know which entry it is scanning
    ixs = {}
    for s, g in sets.items():
        ixs[s] = Indexer.from_gene_slices(g.seqs, g.reversed_flags)
        ixs[s].make_index()
    torch.cuda.synchronize()
    caps = dict(hits_cap=max(1024, n // 16), bytes_cap=max(1024, n // 16) * 2 * L)
    first = ixs[shapes[0]]
    base = lambda ix: scan_pairs_device(ix, *t, L, **caps)                    # noqa: E731
    prep = lambda: prepare_pairs_device(first, *t, L)                         # noqa: E731
    prepared = prep()
    new = lambda ix: scan_prepared_pairs_device(ix, prepared, **caps)         # noqa: E731
    # the same result, per index
    same, totals = True, {}
    for s, ix in ixs.items():
        ra, ba, qa, ta = base(ix).download()
        rb, bb, qb, tb = new(ix).download()
        same = same and ta == tb and ra.tobytes() == rb.tobytes() and ba == bb and qa == qb and ta["overflow"] == 0
        totals[s] = ta
    if a.profile_mode:
        for ix in ixs.values():
            base(ix), new(ix)
        prep()
        torch.cuda.synchronize()
        print(json.dumps({"same_as_scan_pairs_device": same, "totals": totals}))
        return
    for _ in range(a.warmup):
        prep()
        for ix in ixs.values():
            base(ix), new(ix)
    torch.cuda.synchronize()
    ms_a = {s: [] for s in ixs}
    ms_c = {s: [] for s in ixs}
    ms_b = []
    for _ in range(a.repeats):
        ms_b.append(one_call_ms(prep)[0])
        for s, ix in ixs.items():   # (a) and (c) alternate
            ms_a[s].append(one_call_ms(lambda: base(ix))[0])
            ms_c[s].append(one_call_ms(lambda: new(ix))[0])
    med = statistics.median
    tot_a = sum(med(ms_a[s]) for s in shapes)
    tot_c = sum(med(ms_c[s]) for s in shapes)
    b = med(ms_b)
    line = {
        "pairs": n, "read_len": L, "mix": "PANEL", "csvs": K, "shapes": shapes,
        "a_scan_pairs_device_ms": {s: stats(v) for s, v in ms_a.items()},
        "b_prepare_ms": stats(ms_b),
        "c_prepared_scan_ms": {s: stats(v) for s, v in ms_c.items()},
        "d_total_baseline_ms": round(tot_a, 4), "d_total_prepared_ms": round(b + tot_c, 4),
        "d_speedup": round(tot_a / (b + tot_c), 4),
        "c_over_a": {s: round(med(ms_c[s]) / med(ms_a[s]), 4) for s in ixs},
        "e_merged_share": prepared.merged_pairs() / max(n, 1),
        "same_as_scan_pairs_device": same, "totals": totals,
        "retry_slots_prepared": int(mc_lib().gf_mc_retry_capacity(n)),
    }
    print(json.dumps(line))
    for ix in ixs.values():
        ix.close()


if __name__ == "__main__":
    main()
