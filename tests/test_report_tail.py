"""The bulk report tail on the MI355X (genefuserust_amd/report_tail.py, libgfreport.so): the filter reasons against
gf_readmatch_filter, the refined breaks against ``adjust_fusion_break``, the clustering against ``cluster_matches`` and
the independent model, and the file-level scans with ``tail="device"`` against the default."""
import os

import numpy as np
import pytest

from genefuserust_amd import Fusion, GenePos, ReadMatch, _lib, report_tail
from genefuserust_amd.fusion_mapper import FusionMapper
from genefuserust_amd.fusion_result import (FusionResult, Settings, cluster_matches, group_and_sort, report_json,
                                            report_text)
from oracle import indexer_model as model
from tests.helpers import rand_seq, rc
from tests.test_fusion_result import CSV, planted_matches, same, to_model
from tests.test_report_core import adjust_cases, filter_cases, host_filter_reason

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def planted_set(seed):
    """The matches of test_cluster_matches_against_the_model, shuffled: (matches, fusions, genes, fusion sequences)."""
    rng = np.random.default_rng(seed)
    fusions = Fusion.parse_csv_text(CSV)
    seqs = [rand_seq(rng, 6000), rand_seq(rng, 6000), rand_seq(rng, 5000)]
    ms = []
    ms += planted_matches(rng, seqs, 0, 2500, 1, 3100, 9)
    ms += planted_matches(rng, seqs, 1, -3100, 0, -2500, 6)
    ms += planted_matches(rng, seqs, 0, 1200, 2, -900, 5)
    ms += planted_matches(rng, seqs, 0, 1500, 2, 2000, 4)
    ms += planted_matches(rng, seqs, 1, 800, 1, 4000, 5)
    ms += planted_matches(rng, seqs, 0, 4200, 1, 700, 1)
    ms += planted_matches(rng, seqs, 2, 3000, 0, 5000, 5, gap_free=False)
    ms += planted_matches(rng, seqs, 1, 5000, 1, 5001, 4)
    rng.shuffle(ms)
    return ms, fusions, model.csv_genes(CSV), [s.decode() for s in seqs]


def test_filter_reasons(gpu_device):
    """4 096 matches: every boundary case of the core test, among random matches near the thresholds, reads of odd
    lengths so that no read starts where a word does."""
    rng = np.random.default_rng(1)
    cases = [(s, f, thr) for s, f, thr in filter_cases() if thr == 50]
    while len(cases) < 4096:
        n = int(rng.integers(41, 120)) | 1
        seq = rand_seq(rng, n) if rng.random() < 0.8 else (b"A" * (n // 2) + rand_seq(rng, n - n // 2))
        brk = int(rng.integers(15, n - 15)) if rng.random() < 0.95 else int(rng.integers(-3, n + 2))
        lp = int(rng.integers(-300, 300))
        cases.append((seq, (brk, int(rng.integers(0, 4)), int(rng.integers(0, 4)), lp, lp + int(rng.integers(-60, 60)),
                            int(rng.integers(0, 2)), int(rng.integers(0, 2))), 50))
    order = rng.permutation(len(cases))
    cases = [cases[k] for k in order]
    ms = [ReadMatch(s, f[0], GenePos(f[5], f[3]), GenePos(f[6], f[4]), 1, f[1], f[2]) for s, f, _ in cases]
    table = report_tail.MatchTable.from_matches(ms)
    assert (np.diff(table.offsets) % 2 == 1).mean() > 0.9 and (table.offsets % 4 != 0).sum() > 2000
    got = report_tail.filter_reasons_device(table, 50, gpu_device)
    want = np.array([host_filter_reason(s, f, thr) for s, f, thr in cases], dtype=np.int32)
    assert got.dtype == np.int32 and (got == want).all(), np.nonzero(got != want)[0][:10]
    assert set(want.tolist()) == {-1, 0, 1, 2, 3} and (want == 0).sum() > 500
    # FusionMapper.filter_matches' form, on the matches whose break lies inside the read
    inside = [m for m, w in zip(ms, want) if w >= 0]
    kept, removed = report_tail.filter_matches_device(inside, 50, gpu_device)
    counts = np.bincount(want[want >= 0], minlength=4)
    assert removed == {"complexity": counts[1], "distance": counts[2], "indels": counts[3]}
    assert [id(m) for m in kept] == [id(m) for m, w in zip(ms, want) if w == 0]
    with pytest.raises(_lib.GfError):
        report_tail.filter_matches_device(ms, 50, gpu_device)


def check_adjust(frs, device):
    """``adjust_breaks_device`` over all matches of the clusters ``frs`` (fusion point and references made) against
    ``adjust_fusion_break``, field for field."""
    before = [list(fr.m_matches) for fr in frs]
    want = []
    for fr in frs:
        ms = fr.m_matches
        fr.adjust_fusion_break()
        want += [(a.m_read_break - m.m_read_break, a.m_left_distance, a.m_right_distance, 0)
                 for m, a in zip(ms, fr.m_matches)]
    for fr, ms in zip(frs, before):
        fr.m_matches = ms
    flat = [m for ms in before for m in ms]
    cluster = np.repeat(np.arange(len(frs)), [len(ms) for ms in before])
    pieces = [r for fr in frs for r in (fr.m_left_ref, fr.m_right_ref)]
    out = report_tail.adjust_breaks_device(report_tail.MatchTable.from_matches(flat), cluster,
                                           np.frombuffer(b"".join(pieces), dtype=np.uint8),
                                           np.cumsum([0] + [len(p) for p in pieces]), device)
    assert out.shape == (len(flat), 4) and out.dtype == np.int32
    assert out.tolist() == [list(w) for w in want]
    # and through the route's own step, which writes the matches back
    report_tail._adjust_bulk(frs, device)
    for fr, ms in zip(frs, before):
        ref = FusionResult(m_matches=list(ms), m_left_ref=fr.m_left_ref, m_right_ref=fr.m_right_ref)
        ref.adjust_fusion_break()
        assert fr.m_matches == ref.m_matches
        fr.m_matches = ms       # (as they were: the caller's clusters are not refined twice)
    return out


def clusters_of(groups, fseq):
    from genefuserust_amd.fusion_result import first_fit_clusters
    frs = first_fit_clusters(groups)
    for fr in frs:
        fr.calc_fusion_point()
        fr.make_reference(fseq[fr.m_left_gp.contig].encode(), fseq[fr.m_right_gp.contig].encode())
    return frs


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_adjust_on_the_planted_sets(gpu_device, seed):
    ms, fusions, _, fseq = planted_set(seed)
    out = check_adjust(clusters_of(group_and_sort(ms, len(fusions)), fseq), gpu_device)
    assert len(set(out[:, 0].tolist())) >= 3      # the jittered breaks are moved back: several shifts occur


def junction_reads(rng, seqs, n, length, lp=2500, rp=3100):
    """n reads of ``length`` bases across GA's base lp | GB's base rp, breaks anywhere the filter would let through."""
    out = []
    for k in range(n):
        a = int(rng.integers(25, length - 25))
        j = int(rng.integers(-3, 4))
        read = bytearray(seqs[0][lp - a + 1:lp + 1] + seqs[1][rp:rp + length - a])
        for p in rng.integers(0, length, size=max(1, length // 70)):
            read[p] = b"ACGTNa"[int(rng.integers(0, 6))]
        out.append(ReadMatch(bytes(read), a - 1 + j, GenePos(0, lp + j), GenePos(1, rp + j), int(k % 3 != 0), 0, 0,
                             m_name=b"@j%d" % k))
    return out


@pytest.mark.parametrize("length,n", [(150, 300), (250, 200), (1000, 12), (4096, 1)])
def test_adjust_on_read_lengths(gpu_device, length, n):
    rng = np.random.default_rng(length)
    seqs = [rand_seq(rng, 9000), rand_seq(rng, 9000)]
    ms = junction_reads(rng, seqs, n, length, 4500, 4400)
    out = check_adjust(clusters_of([FusionMapper.sort_matches(ms)], [s.decode() for s in seqs]), gpu_device)
    assert (out[:, 3] == 0).all()


def test_adjust_on_the_cores_cases(gpu_device):
    """The cases of the host test of gf_rp_core.h, a cluster each: blocks crossed by the shifts, ties, empty and short
    references, and the matches outside the domain, which come back with their status and through ``_adjust_bulk``
    get ``FusionResult.best_shift``'s answer."""
    cases = adjust_cases()
    frs = [FusionResult(m_matches=[ReadMatch(read, brk, GenePos(0, 500), GenePos(1, 700), 1, 7, 8)], m_left_ref=lref,
                        m_right_ref=rref) for read, brk, lref, rref in cases]
    inside = [fr for fr, (read, brk, _, _) in zip(frs, cases) if 3 <= brk <= len(read) - 5]
    outside = [fr for fr, (read, brk, _, _) in zip(frs, cases) if not 3 <= brk <= len(read) - 5 and -1 <= brk < len(read)]
    check_adjust(inside, gpu_device)
    flat = [fr.m_matches[0] for fr in frs]
    pieces = [r for fr in frs for r in (fr.m_left_ref, fr.m_right_ref)]
    out = report_tail.adjust_breaks_device(report_tail.MatchTable.from_matches(flat), np.arange(len(frs)),
                                           np.frombuffer(b"".join(pieces), dtype=np.uint8),
                                           np.cumsum([0] + [len(p) for p in pieces]), gpu_device)
    want_status = [0 if 3 <= brk <= len(read) - 5 else 1 for read, brk, _, _ in cases]
    assert out[:, 3].tolist() == want_status and 1 in want_status
    assert (out[np.array(want_status) == 1, :3] == 0).all()
    before = [fr.m_matches[0] for fr in outside]
    report_tail._adjust_bulk(outside, gpu_device)
    for fr, m in zip(outside, before):
        ref = FusionResult(m_matches=[m], m_left_ref=fr.m_left_ref, m_right_ref=fr.m_right_ref)
        ref.adjust_fusion_break()
        assert fr.m_matches == ref.m_matches
    # rows that point outside their arrays are a status, not a fault
    table = report_tail.MatchTable.from_matches(flat[:4])
    bad_off = table.offsets.copy()
    bad_off[2] = table.bases.size + 100
    roff = np.cumsum([0] + [len(p) for p in pieces[:8]])
    st = report_tail.adjust_breaks_device(table._replace(offsets=bad_off), [0, 1, 2, 9], np.frombuffer(
        b"".join(pieces[:8]), dtype=np.uint8), roff, gpu_device)[:, 3].tolist()
    assert st == [0, 2, 2, 2]       # (read 1 ends and read 2 starts outside; match 3 names no cluster)
    assert report_tail.filter_reasons_device(table._replace(offsets=bad_off), 50, gpu_device).tolist()[1:3] == [-2, -2]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_cluster_matches_device(gpu_device, seed):
    ms, fusions, genes, fseq = planted_set(seed)
    groups = group_and_sort(ms, len(fusions))
    assert [[id(m) for m in g] for g in group_and_sort(ms, len(fusions), report_tail.order_matches)] == \
        [[id(m) for m in g] for g in groups]
    for st in (Settings(), Settings(output_deletions=True, output_untranslated=True), Settings(unique_requirement=1)):
        want = cluster_matches(groups, fusions, fseq, st)
        got = report_tail.cluster_matches_device(groups, fusions, fseq, st, gpu_device)
        assert len(got) == len(want) > 0
        assert got == want      # every field of every FusionResult, the matches' included
        for g, w in zip(got, want):
            assert g.m_title == w.m_title and (g.m_left_gp, g.m_right_gp) == (w.m_left_gp, w.m_right_gp)
            assert (g.m_left_ref, g.m_right_ref, g.m_left_ref_ext, g.m_right_ref_ext) == \
                (w.m_left_ref, w.m_right_ref, w.m_left_ref_ext, w.m_right_ref_ext) and g.m_unique == w.m_unique
            assert [(m.m_read_break, m.m_left_gp, m.m_right_gp, m.m_left_distance, m.m_right_distance)
                    for m in g.m_matches] == [(m.m_read_break, m.m_left_gp, m.m_right_gp, m.m_left_distance,
                                               m.m_right_distance) for m in w.m_matches]
        assert report_text(got) == report_text(want)
        assert report_json(got, "cmd", "v", "t", st) == report_json(want, "cmd", "v", "t", st)
        mo = model.cluster_model([[to_model(m) for m in g] for g in groups], genes, fseq, st.unique_requirement,
                                 st.output_deletions, st.output_untranslated)
        assert len(got) == len(mo)
        for fr, m in zip(got, mo):
            same(fr, m)


def test_zero_matches_and_a_single_match(gpu_device):
    ms, fusions, _, fseq = planted_set(1)
    assert report_tail.cluster_matches_device([], fusions, fseq, Settings(), gpu_device) == []
    assert report_tail.filter_matches_device([], 50, gpu_device) == ([], {"complexity": 0, "distance": 0, "indels": 0})
    assert report_tail.filter_reasons_device(report_tail.MatchTable.from_matches([]), 50, gpu_device).size == 0
    assert report_tail.adjust_breaks_device(report_tail.MatchTable.from_matches([]), [], np.zeros(0, np.uint8), [0],
                                            gpu_device).shape == (0, 4)
    one = [[ms[0]]]
    st = Settings(unique_requirement=1, output_deletions=True, output_untranslated=True)
    want = cluster_matches(one, fusions, fseq, st)
    assert report_tail.cluster_matches_device(one, fusions, fseq, st, gpu_device) == want
    assert report_tail.cluster_matches_device(one, fusions, fseq, Settings(), gpu_device) == \
        cluster_matches(one, fusions, fseq, Settings()) == []
    assert report_tail.filter_reasons_device(report_tail.MatchTable.from_matches(ms[:1]), 50, gpu_device).tolist() == \
        [host_filter_reason(ms[0].m_read, (ms[0].m_read_break, 0, 0, ms[0].m_left_gp.position,
                                           ms[0].m_right_gp.position, ms[0].m_left_gp.contig,
                                           ms[0].m_right_gp.contig), 50)]


def same_report(a, b):
    assert a[1] == b[1] and list(a[1]) == list(b[1])       # the counters, in their order
    assert a[0] == b[0]
    assert report_json(a[0], "c", "v", "t") == report_json(b[0], "c", "v", "t") and report_text(a[0]) == report_text(b[0])


def test_from_the_golden_files(gpu_device):
    from genefuserust_amd.scan import scan_pair_end_report, scan_single_end_report
    fa, csv = os.path.join(GOLDEN, "tinyref.fa"), os.path.join(GOLDEN, "fusions.csv")
    r1, r2 = os.path.join(GOLDEN, "R1.fq"), os.path.join(GOLDEN, "R2.fq")
    pe = scan_pair_end_report(fa, csv, r1, r2)
    same_report(scan_pair_end_report(fa, csv, r1, r2, tail="device"), pe)
    chunked = scan_pair_end_report(fa, csv, r1, r2, chunk_bytes=1 << 16)
    same_report(scan_pair_end_report(fa, csv, r1, r2, chunk_bytes=1 << 16, tail="device"), chunked)
    assert chunked[0] == pe[0]
    se = scan_single_end_report(fa, csv, r1)
    same_report(scan_single_end_report(fa, csv, r1, tail="device"), se)
    same_report(scan_single_end_report(fa, csv, r1, chunk_bytes=1 << 16, tail="device"),
                scan_single_end_report(fa, csv, r1, chunk_bytes=1 << 16))
    with pytest.raises(ValueError, match="tail"):
        scan_pair_end_report(fa, csv, r1, r2, tail="nope")
    with pytest.raises(ValueError, match="tail"):
        scan_single_end_report(fa, csv, r1, tail="nope")


def test_from_files_with_a_planted_junction(gpu_device, tmp_path):
    """The golden reference holds none of the golden CSV's genes, so those scans end without a match; here the tail
    has matches to filter, sort, cluster and refine: one GA|GB junction under 40 pairs, every route, both tails."""
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report, scan_single_end_report
    rng = np.random.default_rng(21)
    chr1, chr2 = rand_seq(rng, 9000), rand_seq(rng, 8000)
    fa, csv = tmp_path / "ref.fa", tmp_path / "f.csv"
    fa.write_bytes(b">chr1\n" + chr1 + b"\n>chr2\n" + chr2 + b"\n")
    csv.write_text(">GA,chr1:1000-7000\n1,1000,3000\n2,4000,7000\n\n>GB,chr2:500-6500\n1,500,2500\n2,3500,6500\n")
    ga, gb = chr1[1000:7000], chr2[500:6500]
    junction = ga[2300:2600] + gb[3300:3600]
    l_txt, r_txt = [], []
    for k in range(40):
        lo = int(rng.integers(100, 230))
        f = junction[lo:lo + int(rng.integers(200, 270))] if k % 3 == 0 else rand_seq(rng, 260)
        l_txt += [b"@pair%d/1" % k, f[:150], b"+", b"F" * 150]
        r_txt += [b"@pair%d/2" % k, rc(f)[:150], b"+", b"F" * 150]
    r1, r2 = tmp_path / "R1.fq", tmp_path / "R2.fq"
    r1.write_bytes(b"\n".join(l_txt) + b"\n")
    r2.write_bytes(b"\n".join(r_txt) + b"\n")
    args = (str(fa), str(csv), str(r1), str(r2))
    pe = scan_pair_end_report(*args)
    assert len(pe[0]) >= 1 and len(pe[0][0].m_matches) >= 8
    same_report(scan_pair_end_report(*args, tail="device"), pe)
    same_report(scan_pair_end_report(*args, chunk_bytes=4096, tail="device"), scan_pair_end_report(*args, chunk_bytes=4096))
    assert scan_pair_end_files(*args, tail="device") == scan_pair_end_files(*args)
    se = scan_single_end_report(*args[:3])
    assert len(se[0]) >= 1
    same_report(scan_single_end_report(*args[:3], tail="device"), se)
    same_report(scan_single_end_report(*args[:3], chunk_bytes=4096, tail="device"),
                scan_single_end_report(*args[:3], chunk_bytes=4096))
    same_report(scan_report(*args, tail="device"), pe)
    panels = tmp_path / "panels.txt"
    panels.write_text(str(csv) + "\n")
    (_, results, counters), = scan_multi_csv_report(str(fa), str(panels), str(r1), str(r2), tail="device")
    same_report((results, counters), pe)
