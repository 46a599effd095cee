"""libgfmcsv.so on the device: pairs prepared once (gf_mc_pairs_prepare_device) and scanned per index
(gf_mc_pairs_scan_device), byte for byte against gf_scan_pairs_device — the one-call scan — on the same buffers, and for
one gene set against the oracle-driven restatement of the reference's policy; then multi-CSV mode from files against
the single-CSV scanners, entry by entry."""
import json
import os

import numpy as np
import pytest

from tests.helpers import rand_seq, rc

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "branch_cases.json")


def _make_pairs(rng, genes, n, read_len=150, qual=b"E"):
    """As tests/test_pair_pipeline.py makes them: pairs cut from planted fusions (half), one gene or random
    sequence; fragments of 150..300 bases, either strand, some reads with an N or a low quality."""
    g0, g1, g2 = genes[0], genes[1], genes[2]
    pairs = []
    for k in range(n):
        kind = k % 6
        if kind in (0, 1, 2):
            a, b = (g0, g1) if kind != 2 else (g1, g2)
            p, q = int(rng.integers(300, len(a) - 300)), int(rng.integers(300, len(b) - 400))
            frag = a[p - 150:p] + b[q:q + 150]
        elif kind == 3:   # one gene only
            p = int(rng.integers(0, len(g0) - 300))
            frag = g0[p:p + 300]
        else:
            frag = rand_seq(rng, 300)
        lo = int(rng.integers(0, 60))
        flen = int(rng.integers(150, 300 - lo))
        f = frag[lo:lo + flen]
        if k % 2:
            f = rc(f)
        rl = min(read_len, len(f))
        s1, s2 = bytearray(f[:rl]), bytearray(rc(f)[:rl])
        if k % 11 == 0:
            s1[int(rng.integers(0, rl))] = ord("N")
        q1, q2 = bytearray(qual * rl), bytearray(qual * rl)
        if k % 7 == 0:
            q2[int(rng.integers(0, rl))] = ord("#")
        pairs.append((bytes(s1), bytes(q1), bytes(s2), bytes(q2)))
    return pairs


def _ragged(rng, pairs):
    """Ragged lengths, lower case, empty reads, qualities of their own."""
    out = []
    for k, (s1, q1, s2, q2) in enumerate(pairs):
        if k % 3 == 0:
            c1, c2 = len(s1) - k % 40, len(s2) - (k * 7) % 50
            s1, q1, s2, q2 = s1[:c1], q1[:c1], s2[:c2], q2[:c2]
        if k % 5 == 0:
            q1 = bytes(rng.integers(33, 75, size=len(s1), dtype=np.uint8))
            q2 = bytes(rng.integers(33, 75, size=len(s2), dtype=np.uint8))
        if k % 13 == 0:
            s1 = s1.lower()
        if k % 17 == 0:
            s2 = s2[:len(s2) // 2] + s2[len(s2) // 2:].lower()
        if k % 97 == 0:
            s2, q2 = b"", b""
        if k % 389 == 0:
            s1, q1 = b"", b""
        out.append((s1, q1, s2, q2))
    return out


def _upload(pairs):
    import torch
    from genefuserust_amd.read_pair import pack_reads
    lb, lo = pack_reads([p[0] for p in pairs]); lq, _ = pack_reads([p[1] for p in pairs])
    rb, ro = pack_reads([p[2] for p in pairs]); rq, _ = pack_reads([p[3] for p in pairs])
    return [torch.from_numpy(a).cuda() for a in (lb, lq, lo, rb, rq, ro)]


def _golden_genes():
    g = json.load(open(GOLDEN))
    return [None if x is None else x.encode() for x in g["genes"]], list(g["reversed"])


def _same(a, b):
    """(records, bases, qualities, totals) of two scans: every byte."""
    (ra, ba, qa, ta), (rb_, bb, qb, tb) = a, b
    assert ta == tb, (ta, tb)
    assert ra.tobytes() == rb_.tobytes()
    assert ba == bb and qa == qb


def _gene_sets(rng):
    genes, rev = _golden_genes()
    extra = rand_seq(rng, 5000)
    sets = [(genes, rev),
            ([genes[1], genes[0], genes[2], extra], [rev[1], rev[0], rev[2], True]),   # other contig numbers
            ([genes[2], extra, genes[1]], [False, False, True])]                        # gene 0 missing
    return sets


@pytest.mark.gpu
def test_prepared_scan_equals_the_one_call_scan(gpu_device):
    """20 400 pairs prepared ONCE, scanned against three gene sets with three settings of the reversed flags each:
    records (all 64 bytes), hit bases, hit qualities and totals equal gf_scan_pairs_device's on the same buffers."""
    from genefuserust_amd import Indexer
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device, scan_prepared_pairs_device
    from genefuserust_amd.read_pair import scan_pairs_device
    rng = np.random.default_rng(5)
    genes, _ = _golden_genes()
    n = 20_400
    pairs = _ragged(rng, _make_pairs(rng, genes, n))
    assert max(len(p[0]) for p in pairs) == 150 and min(len(p[0]) for p in pairs) == 0
    t = _upload(pairs)
    # hits of every kind are three per pair at most; the synthetic set retries far more reads than a real panel
    caps = dict(hits_cap=3 * n, bytes_cap=2 * int(t[0].numel() + t[3].numel()) + 64, retry_cap=3 * n)
    first = Indexer.from_gene_slices(genes)
    first.make_index()
    prepared = prepare_pairs_device(first, *t, 150)
    first.close()
    seen_sources, seen_rc, seen_retried, seen_merged = set(), 0, 0, 0
    for seqs, rev in _gene_sets(rng):
        for flags in (rev, [False] * len(seqs), [bool(i % 2) for i in range(len(seqs))]):
            ix = Indexer.from_gene_slices(seqs, flags)
            ix.make_index()
            want = scan_pairs_device(ix, *t, 150, pair_id_base=1000, **caps).download()
            got = scan_prepared_pairs_device(ix, prepared, pair_id_base=1000, **caps).download()
            print(len(seqs), flags, want[3])
            assert want[3]["overflow"] == 0 and got[3]["overflow"] == 0
            _same(got, want)
            seen_sources |= {int(s) for s in want[0]["source"]}
            seen_rc = max(seen_rc, int((want[0]["flags"] & 1).sum()))
            seen_retried = max(seen_retried, want[3]["retried_reads"])
            seen_merged = max(seen_merged, want[3]["merged_pairs"])
            assert prepared.merged_pairs() == want[3]["merged_pairs"]
            ix.close()
    # not on empty lists: the one-call scan itself found hits of every kind
    assert seen_sources == {0, 1, 2} and seen_rc >= 50 and seen_retried > 0 and seen_merged >= 300


@pytest.mark.gpu
def test_prepared_buffer_does_not_depend_on_the_index(gpu_device):
    """Prepared with index A, A freed, B built, scanned: gf_scan_pairs_device with B; twice: the same bytes."""
    import torch
    from genefuserust_amd import Indexer
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device, scan_prepared_pairs_device
    from genefuserust_amd.read_pair import scan_pairs_device
    rng = np.random.default_rng(9)
    genes, rev = _golden_genes()
    pairs = _ragged(rng, _make_pairs(rng, genes, 3000))
    t = _upload(pairs)
    a = Indexer.from_gene_slices([rand_seq(rng, 4000), rand_seq(rng, 3000)])
    a.make_index()
    prepared = prepare_pairs_device(a, *t, 150)
    torch.cuda.synchronize()
    a.close()
    b = Indexer.from_gene_slices(genes, rev)
    b.make_index()
    caps = dict(hits_cap=9000, bytes_cap=9000 * 300, retry_cap=9000)
    want = scan_pairs_device(b, *t, 150, **caps).download()
    one = scan_prepared_pairs_device(b, prepared, **caps).download()
    two = scan_prepared_pairs_device(b, prepared, **caps).download()
    assert want[3]["hits"] > 300 and want[3]["overflow"] == 0
    _same(one, want)
    _same(two, one)
    b.close()


def _reference_policy(oracle, ox, rev, pairs):
    """scan_pair_end restated with the oracle (as tests/test_pair_pipeline.py does): per pair the list of (source,
    found_on_rc, m_reversed, read, quality) in push order."""
    def ref_map(seq):
        return oracle.fusion_map_read(ox, rev, seq, ox.map_read(seq))

    def one(seq, qual, source):
        st, _ = ref_map(seq)
        if st == 2:
            return [(source, False, False, seq, qual)]
        if st == 1:
            st, _ = ref_map(rc(seq))
            if st == 2:
                return [(source, True, source != 0, rc(seq), qual[::-1])]
        return []

    out, n_merged = [], 0
    for s1, q1, s2, q2 in pairs:
        m = oracle.fast_merge(s1, q1, s2, q2)
        if m is not None:
            n_merged += 1
            out.append(one(m[0], m[1], 0))
        else:
            out.append(one(s1, q1, 1) + one(s2, q2, 2))
    return out, n_merged


@pytest.mark.gpu
def test_prepared_scan_against_the_oracle_policy(gpu_device, oracle):
    """Independent of every device route: oracle mapping + the reference's policy restated here."""
    from genefuserust_amd import Indexer
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device, scan_prepared_pairs_device
    genes, rev = _golden_genes()
    ix = Indexer.from_gene_slices(genes, rev)
    ix.make_index()
    ox = oracle.OracleIndexer(genes)
    rng = np.random.default_rng(5)
    pairs = _make_pairs(rng, genes, 1500)
    want, n_merged = _reference_policy(oracle, ox, rev, pairs)
    t = _upload(pairs)
    prepared = prepare_pairs_device(ix, *t, 150)
    rec, hb, hq, tot = scan_prepared_pairs_device(ix, prepared, pair_id_base=7, hits_cap=4500, bytes_cap=4500 * 300,
                                                  retry_cap=4500).download()
    assert tot["overflow"] == 0 and tot["merged_pairs"] == n_merged >= 300
    flat = [(p, w) for p, ws in enumerate(want) for w in ws]
    assert tot["hits"] == len(flat) == rec.shape[0] >= 300
    assert tot["retried_reads"] >= sum(1 for _, w in flat if w[1]) >= 50
    for h, (p, (source, on_rc, m_rev, seq, qual)) in zip(rec, flat):
        assert int(h["pair_id"]) == 7 + p and int(h["source"]) == source
        assert bool(h["flags"] & 1) == on_rc and bool(h["flags"] & 2) == m_rev
        o, ln = int(h["seq_offset"]), int(h["read_len"])
        assert hb[o:o + ln] == seq and hq[o:o + ln] == qual
        got = [(int(h["m"][k]["seq_start"]), int(h["m"][k]["seq_end"]), int(h["m"][k]["contig"]),
                int(h["m"][k]["position"])) for k in range(2)]
        assert ox.map_read(seq) == got
    assert {w[0] for _, w in flat} == {0, 1, 2}
    ix.close()


@pytest.mark.gpu
def test_capacities(gpu_device):
    from genefuserust_amd import Indexer
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device, scan_prepared_pairs_device
    from genefuserust_amd.read_pair import scan_pairs_device
    rng = np.random.default_rng(5)
    genes, rev = _golden_genes()
    ix = Indexer.from_gene_slices(genes, rev)
    ix.make_index()
    n = 1500
    pairs = _make_pairs(rng, genes, n)
    t = _upload(pairs)
    full = dict(hits_cap=3 * n, bytes_cap=3 * n * 300)
    want = scan_pairs_device(ix, *t, 150, retry_cap=3 * n, **full).download()
    assert want[3]["overflow"] == 0 and want[3]["retried_reads"] > 8 and want[3]["hits"] > 5
    prepared = prepare_pairs_device(ix, *t, 150)
    # fewer retry slots than retries: bit 1, the count of retries still reported; with room for all: the full result
    small = scan_prepared_pairs_device(ix, prepared, retry_cap=8, **full).download()[3]
    assert small["overflow"] & 1 and small["retried_reads"] == want[3]["retried_reads"]
    _same(scan_prepared_pairs_device(ix, prepared, retry_cap=3 * n, **full).download(), want)
    # fewer records than hits: bit 2, the need reported, the records that fit a prefix of the full list
    few = scan_prepared_pairs_device(ix, prepared, hits_cap=5, bytes_cap=3 * n * 300, retry_cap=3 * n).download()
    assert few[3]["overflow"] == 2 and few[3]["hits"] == want[3]["hits"] and few[3]["hit_bytes"] == want[3]["hit_bytes"]
    assert few[0].shape[0] == 5 and few[0].tobytes() == want[0][:5].tobytes()
    # fewer bytes than the hits' reads: bit 2 again; every record is there, the reads that fit are the first ones
    nb = int(want[0][4]["seq_offset"])
    tight = scan_prepared_pairs_device(ix, prepared, hits_cap=3 * n, bytes_cap=nb, retry_cap=3 * n).download()
    assert tight[3]["overflow"] == 2 and tight[3]["hit_bytes"] == want[3]["hit_bytes"]
    assert tight[0].tobytes() == want[0].tobytes() and tight[1][:nb] == want[1][:nb] and tight[2][:nb] == want[2][:nb]
    ix.close()


@pytest.mark.gpu
def test_long_reads_and_tiny_batches(gpu_device):
    """2 x 250-base pairs: merged reads of more than 320 bases leave the flat kernels for the exact one.  n = 0, 1."""
    import torch
    from genefuserust_amd import Indexer
    from genefuserust_amd.multi_csv_scan import prepare_pairs_device, scan_prepared_pairs_device
    from genefuserust_amd.read_pair import scan_pairs_device
    genes, rev = _golden_genes()
    ix = Indexer.from_gene_slices(genes, rev)
    ix.make_index()
    rng = np.random.default_rng(12)
    g0, g1 = genes[0], genes[1]
    pairs = []
    for k in range(400):
        if k % 4 != 3:
            p, q = int(rng.integers(400, len(g0) - 400)), int(rng.integers(400, len(g1) - 500))
            frag = g0[p - 300:p] + g1[q:q + 300]
        else:
            frag = rand_seq(rng, 600)
        lo = int(rng.integers(0, 100))
        f = frag[lo:lo + int(rng.integers(260, 500))]
        if k % 2:
            f = rc(f)
        rl = min(250, len(f))
        pairs.append((f[:rl], b"F" * rl, rc(f)[:rl], b"F" * rl))
    t = _upload(pairs)
    caps = dict(hits_cap=1200, bytes_cap=1200 * 500, retry_cap=1200)
    want = scan_pairs_device(ix, *t, 250, **caps).download()
    assert want[3]["overflow"] == 0 and want[3]["merged_pairs"] > 100 and want[3]["hits"] > 100
    assert int(((want[0]["source"] == 0) & (want[0]["read_len"] > 320)).sum()) > 20
    _same(scan_prepared_pairs_device(ix, prepare_pairs_device(ix, *t, 250), **caps).download(), want)
    # one pair (a junction pair that does not merge, and one that does), and none
    for k in range(6):
        one = _upload(pairs[k:k + 1])
        w = scan_pairs_device(ix, *one, 250, hits_cap=3, bytes_cap=1500, retry_cap=3).download()
        _same(scan_prepared_pairs_device(ix, prepare_pairs_device(ix, *one, 250), hits_cap=3, bytes_cap=1500,
                                         retry_cap=3).download(), w)
    e = [torch.empty(0, dtype=torch.uint8, device="cuda")] * 2 + [torch.zeros(1, dtype=torch.int64, device="cuda")]
    empty = prepare_pairs_device(ix, *(e + e), 150)
    assert empty.n == 0 and empty.merged_pairs() == 0
    tot = scan_prepared_pairs_device(ix, empty).download()[3]
    assert tot == {"hits": 0, "hit_bytes": 0, "merged_pairs": 0, "retried_reads": 0, "overflow": 0}
    ix.close()


# ---- from files ---------------------------------------------------------------------------------------------------

BLOCKS = {"GA": ">GA,chr1:1000-7000\n1,1000,3000\n2,4000,7000\n",
          "GB": ">GB,chr2:500-6500\n1,500,2500\n2,3500,6500\n",
          "GC": ">GC,chr4:200-5200\n1,200,2200\n2,3200,5200\n",
          "GR": ">GR,chr3:100-5100\n1,3100,5100\n2,100,2100\n"}


def _files(tmp_path):
    """A FASTA of four contigs, the genes GA, GB, GC, GR (GR on the reverse strand) and pairs across two planted
    junctions, GA|GB and GA|GR' (read off GR's other strand), among background pairs; five CSVs of gene subsets and
    a list file naming them (one twice, a blank line in between)."""
    rng = np.random.default_rng(77)
    chrs = {"chr1": rand_seq(rng, 9000), "chr2": rand_seq(rng, 8000), "chr3": rand_seq(rng, 7000),
            "chr4": rand_seq(rng, 6000)}
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">" + k.encode() + b" some description\n" + v + b"\n" for k, v in chrs.items()))
    ga, gb, gr = chrs["chr1"][1000:7000], chrs["chr2"][500:6500], chrs["chr3"][100:5100]
    junctions = [ga[2300 - 300:2300] + gb[3100:3100 + 300],
                 ga[1200 - 300:1200] + rc(gr)[len(gr) - 900:len(gr) - 900 + 300]]
    l_txt, r_txt = [], []
    for k in range(150):
        if k % 3 != 2:
            j = junctions[(k // 3) % 2]
            lo = int(rng.integers(90, 230))
            f = j[lo:lo + int(rng.integers(190, 290))]
            if k % 2:
                f = rc(f)
        else:
            f = rand_seq(rng, 280)
        s1, s2 = bytearray(f[:150]), bytearray(rc(f)[:150])
        q1, q2 = bytearray(b"F" * len(s1)), bytearray(b"F" * len(s2))
        if k % 7 == 0:   # a sequencing error with a low quality
            p = int(rng.integers(5, len(s1) - 5))
            s1[p] = b"ACGT"[(b"ACGT".index(s1[p]) + 1) % 4]
            q1[p] = ord("#")
        if k % 13 == 0:
            s2[int(rng.integers(0, len(s2)))] = ord("N")
        l_txt += [b"@pair%03d/1" % k, bytes(s1), b"+", bytes(q1)]
        r_txt += [b"@pair%03d/2" % k, bytes(s2), b"+", bytes(q2)]
    r1, r2 = tmp_path / "R1.fq", tmp_path / "R2.fq"
    r1.write_bytes(b"\n".join(l_txt) + b"\n")
    r2.write_bytes(b"\n".join(r_txt))   # no final newline, like the reference's own test files
    csvs = {}
    for name, gs in (("ab", ("GA", "GB")), ("agr", ("GA", "GR")), ("none", ("GB", "GC")),
                     ("all", ("GA", "GB", "GC", "GR")), ("ra", ("GR", "GA"))):
        c = tmp_path / (name + ".csv")
        c.write_text("\n".join(BLOCKS[g] for g in gs))
        csvs[name] = str(c)
    order = ["ab", "agr", "none", "all", "ra", "ab"]
    lst = tmp_path / "panels.txt"
    lst.write_text("%s\n%s\n\n  %s\n%s\n%s\n%s\n" % tuple(csvs[k] for k in order))
    return str(fa), str(lst), [csvs[k] for k in order], str(r1), str(r2)


def _texts(results):
    from genefuserust_amd import report_json, report_text
    return report_text(results), report_json(results, "cmd", "0.8.0", "t")


@pytest.mark.gpu
def test_multi_csv_from_files_equals_the_single_csv_scanners(gpu_device, tmp_path):
    from genefuserust_amd.multi_csv_scan import read_csv_list, report_names, scan_multi_csv_report, scan_report
    from genefuserust_amd.scan import scan_pair_end_report, scan_single_end_report
    fa, lst, csvs, r1, r2 = _files(tmp_path)
    assert read_csv_list(lst) == csvs and len(csvs) == 6
    (tmp_path / "out").mkdir()
    jf = str(tmp_path / "out" / "rep.json")
    got = scan_multi_csv_report(fa, lst, r1, r2, json_file=jf, command="cmd", version="0.8.0", time="t")
    assert [g[0] for g in got] == csvs
    alone = {}
    for csv, results, counters in got:
        if csv not in alone:
            alone[csv] = scan_pair_end_report(fa, csv, r1, r2)
        w_results, w_counters = alone[csv]
        print(os.path.basename(csv), counters)
        assert counters == w_counters and counters["pairs"] == 150
        assert _texts(results) == _texts(w_results)
    with_fusions = [g for g in got[:5] if g[2]["fusions"] >= 1]
    assert len(with_fusions) >= 2
    assert len({_texts(g[1])[0] for g in with_fusions}) >= 2            # their result lists differ
    assert got[2][2]["fusions"] == 0 and got[2][1] == []                # GB + GC: nothing planted
    assert got[0][2]["fusions"] >= 1 and got[1][2]["fusions"] >= 1
    assert _texts(got[0][1]) != _texts(got[1][1])
    # the reports, under the names of fusion_scan.rs:190-251; the CSV named twice has one file, holding its report
    names = report_names(jf, csvs)
    assert names[0] == names[5] == str(tmp_path / "out" / "rep_ab.json") and len(set(names)) == 5
    for name, (csv, results, _) in zip(names, got):
        assert open(name).read() == _texts(results)[1]
    # single-end input: against scan_single_end_report
    se = scan_multi_csv_report(fa, lst, r1)
    assert [g[0] for g in se] == csvs
    for csv, results, counters in se:
        w_results, w_counters = scan_single_end_report(fa, csv, r1)
        assert counters == w_counters and counters["reads"] == 150
        assert _texts(results) == _texts(w_results)
    assert sum(1 for g in se if g[2]["fusions"] >= 1) >= 2 and se[2][2]["fusions"] == 0
    # the mode switch
    results, counters = scan_report(fa, csvs[0], r1, r2)
    assert counters == alone[csvs[0]][1] and _texts(results) == _texts(alone[csvs[0]][0])
    results, counters = scan_report(fa, csvs[1], r1)
    w = scan_single_end_report(fa, csvs[1], r1)
    assert counters == w[1] and _texts(results) == _texts(w[0])
    multi = scan_report(fa, lst, r1, r2)
    assert [(c, _texts(r), k) for c, r, k in multi] == [(c, _texts(r), k) for c, r, k in got]
