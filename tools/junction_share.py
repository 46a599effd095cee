"""Does gf_k_probe_buckets' time follow the share of junction reads?  (r07)

Maps 20 M reads of 150 bases against IDX-D with the benchmark's PANEL mix but for the junction share, which is set to
0, 0.1 % (PANEL's own) and 1 % at the background's expense, and prints Indexer.last_stage_ms() — seed+verify, filter,
buckets, exact kernel — averaged over a few calls.  A junction read is one that the bucket pass cannot prove dead: it
was probed to its last window before r07 and leaves the loop as soon as it is safe since.
    python tools/junction_share.py [reads, default 20000000]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from genefuserust_amd import Indexer, synth  # noqa: E402

NAMES = ("gf_k_seedverify_stream", "gf_k_probe_filter", "gf_k_probe_buckets", "gf_k_map_reads_list")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000_000
    L, reps = 150, 5
    genes = synth.make_geneset("IDX-D")
    ix = Indexer.from_gene_slices(genes.seqs, genes.reversed_flags)
    ix.make_index()
    counts = torch.empty(n, dtype=torch.uint8, device="cuda")
    matches = torch.empty((n, 2, 4), dtype=torch.int32, device="cuda")
    for share in (0.0, 0.001, 0.01):
        synth.MIXES["JUNCTION_SHARE"] = (0.401 - share, 0.599, share)
        rb = synth.make_reads(genes, n, read_len=L, mix="JUNCTION_SHARE", seed=20240116, device="cuda")
        for _ in range(2):
            ix.map_reads_device(rb.bases, rb.offsets, L, counts, matches)
        ix.set_profiling(True)
        acc = [0.0] * 4
        for _ in range(reps):
            ix.map_reads_device(rb.bases, rb.offsets, L, counts, matches)
            acc = [a + b for a, b in zip(acc, ix.last_stage_ms())]
        ix.set_profiling(False)
        torch.cuda.synchronize()
        with_segments = int((counts > 0).sum().item())
        print("junction share %.3f %%: reads with segments %d, stage_ms %s" % (
            100 * share, with_segments, {k: round(a / reps, 4) for k, a in zip(NAMES, acc)}), flush=True)
        del rb
    ix.close()


if __name__ == "__main__":
    main()
