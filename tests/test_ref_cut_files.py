"""The reference FASTA cut in chunks on the device (``ref_cut.cut_gene_slices``, ``ref_chunk_bytes`` of the file-level
scans), against the host reader ``FastaReader.read_all`` + ``resolve_gene_slice``: byte for byte the same slices, the
same errors, the same scan results, and neither the host nor the device holds the file."""
import gc
import gzip
import os
import tracemalloc

import numpy as np
import pytest

from genefuserust_amd.indexer import FastaReader, Fusion, Gene, resolve_gene_slice
from tests.helpers import rand_seq
from tests.test_multi_csv_scan import _files, _texts
from tests.test_ref_cut_plan import EDGE_FASTA, EDGE_GENES, _fusions

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CHUNKS = [5, 7, 64, 100, 4096]


def _mirror(path, fusion_lists):
    ref = FastaReader(str(path), True)
    ref.read_all()
    return [[resolve_gene_slice(ref.m_all_contigs, f.m_gene) for f in fl] for fl in fusion_lists]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_cut_of_the_golden_reference_equals_the_mirror(gpu_device, chunk_bytes):
    from genefuserust_amd.ref_cut import cut_gene_slices
    lists = [_fusions([("a", "contig1", 0, 60), ("b", "contig1", 50, 75), ("c", "chrcontig2", 1, 70),
                       ("d", "contig2", 75, 75), ("e", "contig3", 1, 2)]),
             Fusion.parse_csv(os.path.join(GOLDEN, "fusions.csv")),
             _fusions([("f", "contig2", 30, 74)])]
    want = _mirror(os.path.join(GOLDEN, "tinyref.fa"), lists)
    assert want[0][0] and want[0][2] and want[0][4] is None and all(s is None for s in want[1])
    for name in ("tinyref.fa", "tinyref.fa.gz"):
        assert cut_gene_slices(os.path.join(GOLDEN, name), lists, chunk_bytes) == want, name


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", CHUNKS)
def test_cut_of_the_edge_cases_equals_the_mirror(gpu_device, tmp_path, chunk_bytes):
    """Boundaries after '>', inside a name, on the delimiter and inside a gene; two lists in one pass."""
    from genefuserust_amd.ref_cut import cut_gene_slices
    assert 350 < len(EDGE_FASTA) < 500
    fa = tmp_path / "edge.fa"
    fa.write_bytes(EDGE_FASTA)
    lists = [_fusions(EDGE_GENES), _fusions(EDGE_GENES[3:9])]
    want = _mirror(fa, lists)
    assert cut_gene_slices(str(fa), lists, chunk_bytes) == want
    # two concatenated gz members, cut inside a record
    gz = tmp_path / "edge.fa.gz"
    gz.write_bytes(gzip.compress(EDGE_FASTA[:171]) + gzip.compress(EDGE_FASTA[171:]))
    assert _mirror(gz, lists) == want
    assert cut_gene_slices(str(gz), lists, chunk_bytes) == want


@pytest.mark.gpu
def test_error_shapes(gpu_device, tmp_path):
    from genefuserust_amd import _lib
    from genefuserust_amd.ref_cut import cut_gene_slices
    from genefuserust_amd.scan_stream import CARRY_MAX
    fa = tmp_path / "edge.fa"
    fa.write_bytes(EDGE_FASTA)
    # out of range: the host reader's message; on a candidate that loses: no error
    for genes in ([("g", "chr2", 1, 31)], [("g", "chr1", -1, 4)], [("g", "dup", 13, 15)]):
        with pytest.raises(IndexError) as want:
            _mirror(fa, [_fusions(genes)])
        with pytest.raises(IndexError) as e:
            cut_gene_slices(str(fa), [_fusions(genes)], 64)
        assert str(e.value) == str(want.value)
    genes = [("g", "2", 0, 40)]   # "2" holds 40 bytes, "chr2" only 30
    assert cut_gene_slices(str(fa), [_fusions(genes)], 64) == _mirror(fa, [_fusions(genes)])
    # an empty file, plain and zipped; a directory; a file that is not there
    for name, data in (("empty.fa", b""), ("empty.fa.gz", gzip.compress(b""))):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ValueError) as want:
            FastaReader(str(tmp_path / name), True)
        with pytest.raises(ValueError) as e:
            cut_gene_slices(str(tmp_path / name), [[]], 64)
        assert str(e.value) == str(want.value)
    with pytest.raises(IsADirectoryError) as want:
        FastaReader(str(tmp_path), True)
    with pytest.raises(IsADirectoryError) as e:
        cut_gene_slices(str(tmp_path), [[]], 64)
    assert str(e.value) == str(want.value)
    with pytest.raises(FileNotFoundError):
        cut_gene_slices(str(tmp_path / "none.fa"), [[]], 64)
    with pytest.raises(ValueError):
        cut_gene_slices(str(fa), [[]], 0)
    # a name that the carry area cannot hold (longer than the area and a chunk: it is carried unfinished whatever the
    # chunk boundaries): the error names the file; one that just fits is a name like any other
    long_name = tmp_path / "long.fa"
    long_name.write_bytes(b">a\nACGT\n>" + b"n" * (CARRY_MAX + (1 << 18) + 10) + b"\nACGT\n")
    with pytest.raises(_lib.GfError) as e:
        cut_gene_slices(str(long_name), [_fusions([("g", "a", 0, 4)])], 1 << 18)
    assert e.value.code == _lib.GF_ERR_CAPACITY and str(long_name) in str(e.value)
    fits = b"n" * (CARRY_MAX - 1)
    long_name.write_bytes(b">a\nACGT\n>" + fits + b"\nACGTT\n")
    genes = _fusions([("g", "a", 0, 4), ("h", fits.decode(), 1, 5)])
    assert cut_gene_slices(str(long_name), [genes], 1 << 18) == [[b"ACGT", b"CGTT"]]


@pytest.mark.gpu
def test_scans_with_ref_chunk_bytes_equal_the_host_reader(gpu_device, tmp_path):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    from genefuserust_amd.scan import (scan_pair_end_files, scan_pair_end_report, scan_single_end_files,
                                       scan_single_end_report)
    fa, lst, csvs, r1, r2 = _files(tmp_path)
    sets = [(fa, csvs[1], r1, r2, 1000)]
    sets.append(tuple(os.path.join(GOLDEN, n) for n in ("tinyref.fa.gz", "fusions.csv", "R1.fq", "R2.fq")) + (100,))
    for ref, csv, q1, q2, rcb in sets:
        for extra in ({}, {"chunk_bytes": 20_000}):
            res, cnt = scan_pair_end_report(ref, csv, q1, q2, **extra)
            got, gcnt = scan_pair_end_report(ref, csv, q1, q2, ref_chunk_bytes=rcb, **extra)
            assert gcnt == cnt and _texts(got) == _texts(res)
            res, cnt = scan_single_end_report(ref, csv, q1, **extra)
            got, gcnt = scan_single_end_report(ref, csv, q1, ref_chunk_bytes=rcb, **extra)
            assert gcnt == cnt and _texts(got) == _texts(res)
    res, cnt = scan_pair_end_report(fa, csvs[0], r1, r2)
    assert cnt["fusions"] >= 1
    assert scan_single_end_files(fa, csvs[0], r1, route="host", ref_chunk_bytes=999)[1] == \
        scan_single_end_files(fa, csvs[0], r1, route="host")[1]
    got = scan_report(fa, csvs[0], r1, r2, ref_chunk_bytes=1000)
    assert got[1] == cnt and _texts(got[0]) == _texts(res)
    # multi-CSV mode: one pass over the FASTA for all CSVs
    for reads, scan in (((r1, r2), scan_multi_csv_report), ((r1,), scan_report)):
        want = scan_multi_csv_report(fa, lst, *reads)
        got = scan(fa, lst, *reads, ref_chunk_bytes=3000)
        assert [g[0] for g in got] == [w[0] for w in want] == csvs
        for g, w in zip(got, want):
            assert g[2] == w[2] and _texts(g[1]) == _texts(w[1])
    g = os.path.join(GOLDEN, "")
    lst0 = tmp_path / "golden.txt"
    lst0.write_text(g + "fusions.csv\n")
    want = scan_multi_csv_report(g + "tinyref.fa", str(lst0), g + "R1.fq", g + "R2.fq")
    got = scan_multi_csv_report(g + "tinyref.fa", str(lst0), g + "R1.fq", g + "R2.fq", ref_chunk_bytes=7)
    assert [(x[0], _texts(x[1]), x[2]) for x in got] == [(x[0], _texts(x[1]), x[2]) for x in want]
    # remove_alignables needs whole contigs
    with pytest.raises(ValueError) as e:
        scan_pair_end_files(fa, csvs[0], r1, r2, remove_alignables=True, ref_chunk_bytes=1000)
    assert "whole contigs" in str(e.value)


def _synthetic_fasta(path, rng, nbytes: int):
    """Contigs of 256 KiB in lines of 60 letters; a gene of 3000 bases in every one of them."""
    genes, k = [], 0
    line = 61
    with open(path, "wb") as f:
        while f.tell() < nbytes:
            seq = rand_seq(rng, 60 * (1 << 18) // line)
            f.write(b">chr%d\n" % k + b"\n".join(seq[i:i + 60] for i in range(0, len(seq), 60)) + b"\n")
            genes.append(("g%d" % k, "chr%d" % k, 1000 + 7 * k, 4000 + 7 * k))
            k += 1
    return _fusions(genes)


@pytest.mark.gpu
def test_streamed_cut_holds_chunks_not_the_file(gpu_device, tmp_path):
    """Four times the FASTA adds less than one chunk to the device's peak; the host's peak stays below the file's size
    where the host reader's exceeds it."""
    import torch
    from genefuserust_amd.ref_cut import cut_gene_slices
    c = 1 << 20
    rng = np.random.default_rng(21)
    small, big = str(tmp_path / "small.fa"), str(tmp_path / "big.fa")
    genes_small, genes_big = _synthetic_fasta(small, rng, 2 * c), _synthetic_fasta(big, rng, 8 * c)
    size = os.path.getsize(big)
    assert os.path.getsize(small) >= 2 * c and size >= 8 * c

    def host_peak(fn):
        gc.collect()
        tracemalloc.start()
        try:
            out = fn()
            return out, tracemalloc.get_traced_memory()[1]
        finally:
            tracemalloc.stop()

    want, mirror_peak = host_peak(lambda: _mirror(big, [genes_big]))
    assert mirror_peak > size   # (the inputs separate the two readers)
    cut_gene_slices(small, [genes_small], c)   # (warm: what the first call of a process allocates once)

    def device_peak(fn):
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated()

    _, short = device_peak(lambda: cut_gene_slices(small, [genes_small], c))
    (got, cut_peak), long_ = device_peak(lambda: host_peak(lambda: cut_gene_slices(big, [genes_big], c)))
    print("device peak: 2 MiB file %d, 8 MiB file %d; host peak: streamed %d, host reader %d, file %d"
          % (short, long_, cut_peak, mirror_peak, size))
    assert got == want and len(want[0]) >= 32 and all(len(s) == 3000 for s in want[0])
    assert long_ - short < c
    assert cut_peak < size


@pytest.mark.gpu
def test_a_truncated_gz_raises_what_the_host_reader_raises(gpu_device, tmp_path):
    """The inflating upload thread fails in the middle of the file: the cut raises what the host reader raises on that
    file, and the next cut is the mirror's."""
    from genefuserust_amd.ref_cut import cut_gene_slices
    lists = [_fusions(EDGE_GENES)]
    bad, good = tmp_path / "cut_short.fa.gz", tmp_path / "whole.fa.gz"
    bad.write_bytes(gzip.compress(EDGE_FASTA)[:-20])
    good.write_bytes(gzip.compress(EDGE_FASTA))
    with pytest.raises(Exception) as want:
        FastaReader(str(bad), True).read_all()
    with pytest.raises(Exception) as e:
        cut_gene_slices(str(bad), lists, 64)
    assert type(e.value) is type(want.value) and not isinstance(e.value, AssertionError)
    assert cut_gene_slices(str(good), lists, 64) == _mirror(good, lists)
