"""The whole-genome alignable filter on the MI355X (genefuserust_amd/alignable.py, libgfalign.so): the flags of
``alignable_reads_device`` against the brute-force model of the predicate (tests/alignable_model.py), exactly, on a
reference of five contigs (200 to 60 000 bases, 200 kB) and 65 reads (16 to 300 bases and one of 4096) with every case
planted where the kernels can go wrong, at the default piece size (one piece) and at 4096 bytes (some fifty pieces with
overlaps); and one scan from files in which a pair copied whole from elsewhere in the reference is removed by the
filter and by nothing else.

The file's name sorts behind the other GPU tests on purpose: the zero-copy host calls of libgfmatch.so, which are not
touched here, now and then end in "a zero-copy call's kernel ended without reporting completion" once the process has
done other GPU work (seen in tests/test_boundary_gpu.py::test_pack_route_equals_batch_route with these tests in front
of it, and in tests/test_gate_reads.py::test_host_calls[-1] with none of this code run before it), so these tests leave
the order of the others as it was."""
import numpy as np
import pytest

from genefuserust_amd.fusion_mapper import reverse_complement
from tests.alignable_model import WindowIndex
from tests.helpers import rand_seq, rc

LONG = 4096


def other(b: int) -> int:
    return ord("A") if b != ord("A") else ord("C")


def subst(read: bytes, *at: int) -> bytes:
    out = bytearray(read)
    for i in at:
        out[i] = other(out[i])
    return bytes(out)


def flip(s: bytes) -> bytes:
    return bytes(other(b) for b in s)


def build_world():
    """(reference, [(label, read)]).  With 4096-byte pieces and the long read, contig c0 is cut into pieces of 8192
    bytes that start every 4097 bases; without it, into pieces of 4096 that start every 3797."""
    rng = np.random.default_rng(2026)
    unit = rand_seq(rng, 41)
    c0 = bytearray(rand_seq(rng, 60000))
    c1 = rand_seq(rng, 200)
    c2 = bytearray(rand_seq(rng, 50000))
    c2[7000:9050] = (unit * 51)[:2050]                      # a 2 kB tandem repeat
    c2[20000:20400] = bytes(c2[20000:20400]).lower()        # a lower-case stretch
    c2[30000:30009] = b"N" * 9                              # N runs of 9 and 10 bases
    c2[31000:31010] = b"N" * 10
    c3 = rand_seq(rng, 30000)
    c4 = rand_seq(rng, 59800)
    c0, c2 = bytes(c0), bytes(c2)
    reference = {"c0": c0, "c1": c1, "c2": c2, "c3": c3, "c4": c4}
    base = c3[10000:10200]
    L = len(base)
    far = c3[25000:25200]
    R = [
        # the table of the specification
        ("exact copy", base),
        ("reverse-complement copy", reverse_complement(base)),
        ("lower-case reference", c2[20100:20300].upper()),
        ("substitution at 8", subst(base, 8)),
        ("substitution at 9", subst(base, 9)),
        ("substitution at L - 9", subst(base, L - 9)),
        ("substitution at L - 10", subst(base, L - 10)),
        ("two substitutions 8 apart", subst(base, 100, 108)),
        ("two substitutions 10 apart", subst(base, 100, 110)),
        ("fusion read 100 + 100", base[:100] + far[:100]),
        ("191 + 9", base[:191] + flip(base[191:])),
        ("190 + 10 substituted", base[:190] + flip(base[190:])),
        ("across the junction of two contigs", c0[-100:] + c1[:100]),
        ("across the junction, the next pair", c1[-100:] + c2[:100]),
        ("the same length inside one contig", c0[-200:]),
        ("25-base exact copy", base[:25]),
        ("15-base exact copy", base[:15]),
        ("16-base exact copy", c4[777:793]),
        ("26-base copy, reverse strand", reverse_complement(c4[5000:5026])),
        # the ends of contigs, and a contig that is one read
        ("copy at p = 0", c0[:150]),
        ("copy at p = 0, reverse strand", reverse_complement(c3[:120])),
        ("copy at p = len - L", c4[-150:]),
        ("copy at p = len - L of the first contig", c0[-300:]),
        ("a whole contig", c1),
        ("a whole contig and one base more", c1 + b"A"),
        # piece boundaries of contig c0 at 4096-byte pieces, with and without the long read
        ("across the end of the first 8192-byte piece", c0[8100:8300]),
        ("across the start of the second 8192-byte piece", c0[4000:4200]),
        ("across the end of the first 4096-byte piece", c0[3996:4196]),
        ("ends with the first 4096-byte piece", c0[3896:4096]),
        ("starts with the second 4096-byte piece", c0[3797:3997]),
        ("300 bases across a cut", c0[12100:12400]),
        # the tandem repeat: one key with a long equal range, one diagonal with many exact runs
        ("from the tandem repeat", c2[7500:7700]),
        ("from the tandem repeat, substitutions every 20", subst(c2[7500:7700], *range(10, 200, 20))),
        ("from the tandem repeat, substitutions every 17", subst(c2[7500:7740], *range(5, 240, 17))),
        ("out of the tandem repeat's end", c2[8950:9150]),
        ("units of the repeat", unit * 7 + unit[:13]),
        # reads that share their 16-mers
        ("shares all 16-mers but the last", c4[30000:30100]),
        ("shares all 16-mers but the last, other one", subst(c4[30000:30100], 99)),
        ("shares all 16-mers but the first", subst(c4[30000:30100], 0)),
        # N, case, strands
        ("read with an N", base[:60] + b"N" + base[61:]),
        ("read with an N at 9", base[:9] + b"N" + base[10:]),
        ("lower-case read", base.lower()),
        ("over 9 Ns of the reference", c2[29950:30150]),
        ("over 10 Ns of the reference", c2[30950:31150]),
        ("its own reverse complement", None),
        ("random", rand_seq(rng, 150)),
        ("poly-A", b"A" * 60),
        ("empty", b""),
    ]
    own = c4[40000:40050]
    R = [(k, own + reverse_complement(own) if r is None else r) for k, r in R]
    # (a palindrome is in the reference only if planted: it is not, so the model says no unless chance has it)
    contigs = [c0, c2, c3, c4]
    while len(R) < 64:   # random reads drawn from the reference with 0 .. 12 substitutions at random places
        c = contigs[int(rng.integers(0, 4))]
        n = int(rng.integers(16, 301))
        p = int(rng.integers(0, len(c) - n))
        r = bytearray(c[p:p + n].upper())
        for i in rng.integers(0, n, int(rng.integers(0, 13))).tolist():
            r[i] = other(r[i])
        R.append(("random draw %d" % len(R), reverse_complement(bytes(r)) if rng.integers(0, 2) else bytes(r)))
    long_read = subst(c0[20000:20000 + LONG], 5, 1000, 3000, LONG - 1)    # 9 uncovered
    R.append(("4096 bases", long_read))
    return reference, R


@pytest.fixture(scope="module")
def world():
    reference, labelled = build_world()
    reads = [r for _, r in labelled]
    assert len(reads) == 65 and sum(len(c) for c in reference.values()) == 200_000
    assert len(reference) == 5 and max(len(r) for r in reads[:-1]) == 300 and len(reads[-1]) == LONG
    want = WindowIndex(reference).alignable_reads(reads)
    want.setflags(write=False)
    return reference, [k for k, _ in labelled], reads, want


def _mismatches(labels, got, want):
    return [(k, bool(g), bool(w)) for k, g, w in zip(labels, got, want) if g != w]


def test_the_model_decides_the_planted_cases_as_the_specification_says(world):
    """No GPU: what the GPU tests below compare with is the specification's table."""
    _, labels, _, want = world
    says = dict(zip(labels, want.tolist()))
    yes = ["exact copy", "reverse-complement copy", "lower-case reference", "substitution at 8", "substitution at L - 9",
           "two substitutions 8 apart", "191 + 9", "the same length inside one contig", "25-base exact copy",
           "16-base exact copy", "26-base copy, reverse strand", "copy at p = 0", "copy at p = len - L", "a whole contig",
           "across the end of the first 8192-byte piece", "across the end of the first 4096-byte piece",
           "from the tandem repeat", "shares all 16-mers but the last", "shares all 16-mers but the last, other one",
           "read with an N", "over 9 Ns of the reference", "4096 bases"]
    no = ["substitution at 9", "substitution at L - 10", "two substitutions 10 apart", "fusion read 100 + 100",
          "190 + 10 substituted", "across the junction of two contigs", "across the junction, the next pair",
          "15-base exact copy", "a whole contig and one base more", "from the tandem repeat, substitutions every 20",
          "read with an N at 9", "lower-case read", "over 10 Ns of the reference", "random", "poly-A", "empty"]
    assert [k for k in yes if not says[k]] == [] and [k for k in no if says[k]] == []


@pytest.mark.gpu
@pytest.mark.parametrize("batch_bytes,with_long", [(256 << 20, True), (4096, True), (4096, False)],
                         ids=["one piece", "8192-byte pieces", "4096-byte pieces"])
def test_flags_equal_the_model(gpu_device, world, batch_bytes, with_long):
    from genefuserust_amd.alignable import alignable_reads_device
    reference, labels, reads, want = world
    n = len(reads) if with_long else len(reads) - 1
    stats = {}
    got = alignable_reads_device(reference, reads[:n], gpu_device, batch_bytes, stats=stats)
    print("alignable: %d of %d reads, %d pieces, %d seeds, scan %.3f ms" % (
        int(got.sum()), n, stats["pieces"], stats["seeds"], sum(stats["scan_ms"])))
    assert got.dtype == bool and got.shape == (n,)
    assert _mismatches(labels, got, want[:n]) == []
    if batch_bytes == 4096:   # pieces of max(4096, 2 x the longest read) bytes, overlapping by the longest read less one
        from genefuserust_amd.alignable import plan_pieces
        piece, overlap = (8192, LONG - 1) if with_long else (4096, 299)
        assert stats["pieces"] == len(plan_pieces([len(c) for c in reference.values()], piece, overlap)) > 40
        assert stats["text_bytes"] > 200_000
    else:
        assert stats["pieces"] == 1 and stats["text_bytes"] == 200_000 + 4
    assert 15 < int(want.sum()) < 50


@pytest.mark.gpu
def test_two_runs_and_every_filter_size_give_equal_flags(gpu_device, world):
    from genefuserust_amd.alignable import alignable_reads_device
    reference, labels, reads, want = world
    first = alignable_reads_device(reference, reads, gpu_device, 32768)
    assert _mismatches(labels, first, want) == []
    assert (alignable_reads_device(reference, reads, gpu_device, 32768) == first).all()
    # 2^16 bits are half full with these reads' keys (false positives reach the seed table); 2^32 is the exact map
    for bits in (16, 21, 32):
        assert (alignable_reads_device(reference, reads, gpu_device, 32768, filter_log2_bits=bits) == first).all(), bits
    # the order of the reads does not matter, nor does the company they are in
    order = np.random.default_rng(1).permutation(len(reads))
    assert (alignable_reads_device(reference, [reads[i] for i in order], gpu_device)[np.argsort(order)] == first).all()
    for i in (0, 9, 31, 64):
        assert alignable_reads_device(reference, reads[i:i + 1], gpu_device).tolist() == [bool(want[i])], labels[i]


@pytest.mark.gpu
def test_no_reference_no_reads_and_bytes_of_every_kind(gpu_device, world):
    from genefuserust_amd.alignable import alignable_reads_device
    reference, _, reads, want = world
    assert alignable_reads_device(None, reads, gpu_device).tolist() == [False] * len(reads)
    assert alignable_reads_device({"c": b""}, reads[:3], gpu_device).tolist() == [False] * 3
    assert alignable_reads_device(reference, [], gpu_device).shape == (0,)
    # a reference shorter than a window, one of exactly a window, and bytes outside the alphabet on both sides
    assert alignable_reads_device({"c": b"ACGTACGTACGTACG"}, [b"ACGTACGTACGTACGT"], gpu_device).tolist() == [False]
    tiny = {"a": b"ACGTTGCATTGACCAG", "b": bytes(range(256)), "c": b"acgttgcattgaccagT"}
    odd = [b"ACGTTGCATTGACCAG", b"CTGGTCAATGCAACGT", bytes(range(256)), b"ACGTTGCATTGACCAGT", b"\0" * 40, b"N" * 40]
    assert alignable_reads_device(tiny, odd, gpu_device).tolist() == WindowIndex(tiny).alignable_reads(odd).tolist() \
        == [True, True, False, True, False, False]
    # bytearray contigs, as a FASTA reader may hand them over
    assert (alignable_reads_device({k: bytearray(v) for k, v in reference.items()}, reads[:20], gpu_device)
            == want[:20]).all()


def _planted_files(tmp_path):
    """tests/test_multi_csv_scan.py's planted-fusion files, plus one pair that looks like a GA|GB fusion at a junction
    of its own and is copied whole from a fifth contig, where that chimeric stretch stands."""
    from genefuserust_amd.scan import read_contigs
    from tests.test_multi_csv_scan import _files
    fa, _, csvs, r1, r2 = _files(tmp_path)
    chrs = read_contigs(fa)
    ga, gb = bytes(chrs["chr1"])[1000:7000], bytes(chrs["chr2"])[500:6500]
    junction = ga[4800 - 300:4800] + gb[1500:1500 + 300]
    rng = np.random.default_rng(5)
    with open(fa, "ab") as f:
        f.write(b">chr5 a paralogue\n" + rand_seq(rng, 1500) + junction[150:450] + rand_seq(rng, 1500) + b"\n")
    frag = junction[200:400]
    with open(r1, "ab") as f:
        f.write(b"@planted/1\n" + frag[:150] + b"\n+\n" + b"F" * 150 + b"\n")
    with open(r2, "ab") as f:
        f.write(b"\n@planted/2\n" + rc(frag)[:150] + b"\n+\n" + b"F" * 150)
    return fa, csvs[0], r1, r2


def _key(m):
    return (m.m_name, bytes(m.m_read), m.m_read_break, m.m_left_gp.contig, m.m_left_gp.position, m.m_right_gp.contig,
            m.m_right_gp.position, m.m_reversed)


@pytest.mark.gpu
@pytest.mark.parametrize("tail", ["host", "device"])
def test_a_pair_copied_from_elsewhere_in_the_reference_is_removed_and_nothing_else_moves(gpu_device, tmp_path, tail):
    from genefuserust_amd.scan import read_contigs, scan_pair_end_files, scan_pair_end_report
    from tests.test_multi_csv_scan import _texts
    fa, csv, r1, r2 = _planted_files(tmp_path)
    kept, counters = scan_pair_end_files(fa, csv, r1, r2, gpu_device, tail=tail)
    planted = [m for m in kept if m.m_name.startswith(b"@planted")]
    assert 1 <= len(planted) <= 2 and counters["pairs"] == 151 and "genome_alignables" not in counters
    # the model: of the matches the other filters keep, the planted pair's reads are alignable and no other is
    index = WindowIndex(read_contigs(fa))
    assert [index.alignable(bytes(m.m_read)) for m in kept] == [m.m_name.startswith(b"@planted") for m in kept]
    filtered, with_filter = scan_pair_end_files(fa, csv, r1, r2, gpu_device, tail=tail, alignable_filter="genome")
    assert [_key(m) for m in filtered] == [_key(m) for m in kept if not m.m_name.startswith(b"@planted")]
    assert len(filtered) >= 10   # (the comparison above is not of two empty lists)
    assert with_filter == {**counters, "genome_alignables": len(planted)}
    order = list(counters)
    assert list(with_filter) == order[:order.index("indels") + 1] + ["genome_alignables"] + order[order.index("indels") + 1:]
    # the report: the planted pair alone supports no fusion, so the fusions are the same, to the byte
    res, cnt = scan_pair_end_report(fa, csv, r1, r2, gpu_device, tail=tail)
    res_f, cnt_f = scan_pair_end_report(fa, csv, r1, r2, gpu_device, tail=tail, alignable_filter="genome")
    names = [m.m_name for fr in res for m in fr.m_matches]
    assert [m.m_name for fr in res_f for m in fr.m_matches] == [nm for nm in names if not nm.startswith(b"@planted")]
    assert cnt_f == {**cnt, "genome_alignables": len(planted), "fusions": len(res_f)} and len(res_f) >= 1
    if not any(nm.startswith(b"@planted") for nm in names):
        assert _texts(res_f) == _texts(res) and cnt_f["fusions"] == cnt["fusions"]
