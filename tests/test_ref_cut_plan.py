"""The planning of the reference cut (genefuserust_amd/ref_cut.py: ``CutPlan``, ``plan_chunk``, ``CutPass``) without a
GPU, against the host mirror ``FastaReader.read_all`` + ``resolve_gene_slice``.  The two device calls are replaced by a
plain host loop over the chunk's bytes (``model_index``, ``model_gather``: the rules of include/gf_ref_cut.h restated),
which tests/test_ref_cut_abi.py compares the device with."""
import numpy as np
import pytest

from genefuserust_amd.indexer import FastaReader, Fusion, Gene, resolve_gene_slice

KEEP = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz-*")


def _fusions(genes):
    return [Fusion(Gene(name, chr_, start, end)) for name, chr_, start, end in genes]


def model_index(text: bytes):
    """What gf_rc_index_device + ``RefIndex.download`` give for ``text``, byte by byte on the host."""
    from genefuserust_amd.ref_cut import ChunkRecords
    rank = np.concatenate([[0], np.cumsum([c in KEEP for c in text])]).astype(np.int64)
    gt_pos = [p for p, c in enumerate(text) if c == ord(">")]
    name_end, seq_rank, names = [], [], []
    for k, g in enumerate(gt_pos):
        end = gt_pos[k + 1] if k + 1 < len(gt_pos) else len(text)
        at = next((p for p in range(g + 1, end) if text[p] in b"\n "), -1)
        name_end.append(at)
        seq_rank.append(rank[at + 1] if at >= 0 else rank[end])
        names.append(text[g + 1:at if at >= 0 else end])
    unfinished = gt_pos[-1] if gt_pos and name_end[-1] < 0 else -1
    as64 = lambda x: np.array(x, dtype=np.int64)
    return ChunkRecords(len(gt_pos), int(rank[-1]), unfinished, as64(gt_pos), as64([rank[g] for g in gt_pos]),
                        as64(name_end), as64(seq_rank), names)


def model_gather(text: bytes, rec, n_records: int, rows, out_bytes: int, carried_kept: int = 0, fill: int = 0) -> bytes:
    """What gf_rc_gather_device leaves in an output of ``out_bytes`` bytes that held ``fill``."""
    out = bytearray([fill]) * out_bytes
    r, base, rank = 0, -carried_kept, 0
    for c in text:
        if c == ord(">"):
            r += 1
            if r > n_records:
                break
            base = int(rec.seq_rank[r - 1])
        elif c in KEEP:
            pos, rank = rank - base, rank + 1
            for k, s, e, off in rows:
                if k == r and s <= pos < e and 0 <= off + pos - s < out_bytes:
                    out[off + pos - s] = ord(chr(c).upper())
    return bytes(out)


def model_cut(text: bytes, fusion_lists, chunk_bytes: int):
    """``cut_gene_slices`` with the device replaced by the model: the same ``CutPass`` per chunk, the same carry."""
    from genefuserust_amd.ref_cut import CutPass, CutPlan
    plan = CutPlan(fusion_lists)
    state, carry, pos = CutPass(plan), b"", 0
    while True:
        chunk = carry + text[pos:pos + chunk_bytes]
        pos += chunk_bytes
        final = pos >= len(text)
        rec = model_index(chunk)
        done = state.chunk(rec, len(chunk), final, lambda n, nbytes, rows, total, carried: model_gather(
            chunk[:nbytes], rec, n, rows, total, carried))
        carry = chunk[done:]
        if final:
            return plan.finish()


def mirror(tmp_path, text: bytes, fusion_lists, name="ref.fa"):
    """The yardstick: the host reader on a file that holds ``text``.  (slices, None) or (None, the exception)."""
    path = tmp_path / name
    path.write_bytes(text)
    ref = FastaReader(str(path), True)
    ref.read_all()
    try:
        return [[resolve_gene_slice(ref.m_all_contigs, f.m_gene) for f in fl] for fl in fusion_lists], None
    except IndexError as e:
        return None, e


# the edge cases of the FASTA rules in about 400 bytes: text before the first '>', a description that becomes sequence,
# "\r\n" line ends, lower case, '-', '*', digits, a '>' inside a header line, an empty record, duplicate names, a name
# that "chr" + name and the name without "chr" resolve to, no final newline
EDGE_FASTA = (b"junk ACGT before\n>chr1 a description\nACGTacgtNN\nGGGG-*cc\r\nTTTT1234AAAA\n"
              b">5\tnot a blank\nACGTACGTACGTACGTACGTACGTACGTAC\nTTGGCCAATTGGCCAATTGGCCAATTGGCC\n"
              b">2\nCCCCCCCCCCGGGGGGGGGG\nAAAAAAAAAATTTTTTTTTT\n>chr2\nTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT\n"
              b">odd>inner rest\nACGTACGT\n>\n>chr3\r\nACGTTGCA\r\nacgttgca\r\n>dup\nAAAAAAAAAAAA\n>dup\nCCCCCCCCCCCCGG\n"
              b">chrchr4\nGATTACAGATTACA\n>4\nTTTTGGGGCCCCAAAA\n>X\nacgtnACGTN\n>chrX\nGGGGGGGGGG\n>last\nACGTACGTAC")
EDGE_GENES = [
    ("g_desc", "chr1", 2, 20), ("g_desc2", "1", 0, 5), ("g_overlap", "chr1", 10, 30), ("g_touch", "chr1", 30, 33),
    ("g_exact_over_chr", "2", 5, 25), ("g_chr2", "chr2", 1, 30), ("g_inner", "inner", 3, 11), ("g_odd", "odd", 0, 0),
    ("g_crlf", "3", 4, 16), ("g_dup", "dup", 2, 14), ("g_strike_twice", "chrchr4", 4, 12), ("g_strike", "chr4", 1, 14), ("g_struck", "chr4chr", 1, 16),
    ("g_x", "X", 1, 10), ("g_chrx", "chrX", 1, 10), ("g_last", "last", 5, 10), ("g_missing", "chr9", 1, 5),
    ("g_empty_name", "", 0, 0), ("g_tab_name", "5\tnot", 25, 45), ("g_no_tab", "5", 25, 45),
]


def _feed(plan, records):
    """Whole records, in file order, into a plan."""
    for name, seq in records:
        c = plan.start_record(name)
        if c is not None:
            for i, s, e in c.wanted(0, len(seq)):
                c.put(i, s, seq[s:e])
            c.length = len(seq)


def _plan_slices(records, genes):
    from genefuserust_amd.ref_cut import CutPlan
    plan = CutPlan([_fusions(genes)])
    _feed(plan, records)
    return plan.finish()[0]


def _host_slices(records, genes):
    contigs = dict(records)   # (the last of duplicate names wins, as in read_all)
    return [resolve_gene_slice(contigs, f.m_gene) for f in _fusions(genes)]


def test_precedence_of_the_three_name_forms():
    from genefuserust_amd.ref_cut import candidate_names
    assert candidate_names("1") == ["1", "chr1"]
    assert candidate_names("chr1") == ["chr1", "chrchr1", "1"]
    assert candidate_names("chrchr1") == ["chrchr1", "chrchrchr1", "1"]   # replace strikes twice
    a, b, c = b"AAAAAAAAAA", b"CCCCCCCCCC", b"GGGGGGGGGG"
    genes = [("g", "chr1", 2, 8)]
    for records in ([("1", a), ("chrchr1", b), ("chr1", c)], [("1", a), ("chrchr1", b)], [("1", a)],
                    [("chrchr1", b), ("1", a)]):
        assert _plan_slices(records, genes) == _host_slices(records, genes)
    assert _plan_slices([("1", a), ("chrchr1", b), ("chr1", c)], genes) == [c[2:8]]
    assert _plan_slices([("1", a), ("chrchr1", b)], genes) == [b[2:8]]
    assert _plan_slices([("1", a)], genes) == [a[2:8]]
    genes = [("g", "chrchr1", 0, 3)]
    records = [("1", a), ("chr1", c)]   # "chrchr1" without its "chr"s is "1", never "chr1"
    assert _plan_slices(records, genes) == _host_slices(records, genes) == [a[:3]]


def test_chr_plus_name_earlier_in_the_file_than_the_exact_name():
    genes = [("g", "7", 1, 6)]
    records = [("chr7", b"ACGTACGTAC"), ("other", b"TTTT"), ("7", b"GGGGGCCCCC")]
    assert _plan_slices(records, genes) == _host_slices(records, genes) == [b"GGGGC"]
    assert _plan_slices(records[:2], genes) == _host_slices(records[:2], genes) == [b"CGTAC"]


def test_the_last_of_duplicate_names_wins():
    genes = [("g", "7", 1, 6), ("h", "chr7", 0, 12)]
    records = [("7", b"ACGTACGTAC"), ("chr7", b"AAAAAAAAAAAAAAA"), ("7", b"GGGGGCCCCCTT")]
    assert _plan_slices(records, genes) == _host_slices(records, genes) == [b"GGGGC", b"AAAAAAAAAAAA"]
    # the last one is shorter than the range: the earlier, long enough one does not help
    short = records + [("chr7", b"AAAA")]
    with pytest.raises(IndexError) as e:
        _plan_slices(short, genes)
    with pytest.raises(IndexError) as want:
        _host_slices(short, genes)
    assert str(e.value) == str(want.value) == "gene h: range 0..12 outside contig chr7 (len 4)"


def test_merging_and_unmerging():
    from genefuserust_amd.ref_cut import CutPlan, merge_ranges
    assert merge_ranges([(5, 9), (1, 3), (3, 4), (8, 12), (20, 20), (-1, 4), (7, 6), (30, 31)]) == [(1, 4), (5, 12), (30, 31)]
    assert merge_ranges([]) == [] and merge_ranges([(0, 0)]) == []
    seq = bytes(np.random.default_rng(1).choice(list(b"ACGT"), 200).astype(np.uint8))
    lists = [[("a", "c", 10, 50), ("b", "c", 40, 90), ("c", "c", 90, 100), ("d", "c", 150, 160)],
             [("e", "chrc", 45, 95), ("f", "c", 10, 50), ("g", "c", 199, 200), ("h", "c", 120, 120)]]
    plan = CutPlan([_fusions(g) for g in lists])
    assert plan.intervals["c"] == [(10, 100), (150, 160), (199, 200)]
    assert plan.intervals["chrc"] == [(10, 100), (150, 160), (199, 200)] and plan.intervals["chrchrc"] == [(45, 95)]
    c = plan.start_record("c")
    assert c.wanted(0, 200) == [(0, 10, 100), (1, 150, 160), (2, 199, 200)]
    assert c.wanted(60, 155) == [(0, 60, 100), (1, 150, 155)] and c.wanted(100, 150) == [] and c.wanted(160, 199) == []
    # the bytes arrive in pieces, as from chunks that end inside a gene
    for lo, hi in ((0, 7), (7, 60), (60, 155), (155, 200)):
        for i, s, e in c.wanted(lo, hi):
            c.put(i, s, seq[s:e])
        c.length = hi
    got = plan.finish()
    assert got == [[seq[s:e] for _, _, s, e in g] for g in lists]
    assert got[1][3] == b""


def test_ranges_at_the_contigs_end_and_outside_it():
    seq = b"ACGTACGTAC"
    records = [("c", seq)]
    assert _plan_slices(records, [("g", "c", 4, 10)]) == [seq[4:10]]          # end == len
    assert _plan_slices(records, [("g", "c", 10, 10)]) == [b""]              # start == end == len
    assert _plan_slices(records, [("g", "c", 3, 3)]) == [b""]
    for genes in ([("g", "c", 4, 11)], [("g", "c", -2, 4)], [("g", "c", 6, 4)], [("g", "c", 11, 11)]):
        with pytest.raises(IndexError) as e:
            _plan_slices(records, genes)
        with pytest.raises(IndexError) as want:
            _host_slices(records, genes)
        assert str(e.value) == str(want.value)
    # out of range only on a candidate that loses: no error, here or in the mirror
    records = [("chrc", b"ACGT"), ("c", seq)]
    genes = [("g", "c", 4, 10)]
    assert _plan_slices(records, genes) == _host_slices(records, genes) == [seq[4:10]]
    # and the chosen one is checked even when a losing one would do
    records = [("chrc", seq), ("c", b"ACGT")]
    with pytest.raises(IndexError) as e:
        _plan_slices(records, genes)
    assert str(e.value) == "gene g: range 4..10 outside contig c (len 4)"


def test_a_missing_chromosome_gives_none():
    records = [("c", b"ACGTACGT")]
    genes = [("g", "d", 1, 4), ("h", "c", 1, 4), ("i", "chrd", 100, 200)]
    assert _plan_slices(records, genes) == _host_slices(records, genes) == [None, b"CGT", None]


@pytest.mark.parametrize("chunk_bytes", [1, 5, 7, 64, 100, 4096])
def test_chunked_pass_over_the_edge_cases_equals_the_mirror(tmp_path, chunk_bytes):
    """``CutPass`` over the model of the device, chunk boundaries after '>', inside a name, on the delimiter and
    inside a gene: the slices of the host reader."""
    lists = [_fusions(EDGE_GENES), _fusions(EDGE_GENES[3:9])]
    want, err = mirror(tmp_path, EDGE_FASTA, lists)
    assert err is None and want[0][0] == b"ESCRIPTIONACGTACGT" and want[0][16] is None
    assert model_cut(EDGE_FASTA, lists, chunk_bytes) == want


@pytest.mark.parametrize("text", [b">", b">a", b">a\n", b"no record at all\nACGT\n", b">a\nACGT>", b">a\nAC>>b\nGG>\n",
                                  b">a b>a\nTT", b"\n\n>a\r\nAC\r\n\r\n"])
def test_chunked_pass_over_small_texts_equals_the_mirror(tmp_path, text):
    lists = [_fusions([("g", "a", 0, 2), ("h", "b", 0, 2), ("i", "", 0, 0)])]
    want, err = mirror(tmp_path, text, lists)
    for chunk_bytes in (1, 2, 3, 100):
        if err is not None:
            with pytest.raises(IndexError) as e:
                model_cut(text, lists, chunk_bytes)
            assert str(e.value) == str(err)
        else:
            assert model_cut(text, lists, chunk_bytes) == want
