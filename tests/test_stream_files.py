"""The streamed file-level scans (scan_stream.py, hit_names.py, scan.py with ``chunk_bytes``) on the device: the names
of the hit records against the host text, the single-end stream against the one-shot scan and the oracle, the
file-level scans in chunks against the whole-file route, and the memory a streamed scan holds."""
import gc
import gzip
import json
import os

import numpy as np
import pytest

from tests.helpers import rand_seq, rc
from tests.test_multi_csv_scan import _files, _texts
from tests.test_pair_pipeline import _make_pairs
from tests.test_single_end_device import _quals_for, _synthetic

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "branch_cases.json")


def _golden_index():
    from genefuserust_amd import Indexer
    g = json.load(open(GOLDEN))
    genes = [None if x is None else x.encode() for x in g["genes"]]
    ix = Indexer.from_gene_slices(genes, g["reversed"])
    ix.make_index()
    return ix, genes


def _device_text(text: bytes):
    import torch
    return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()


# ---- 1. names against the host ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("final_newline", [True, False])
def test_names_of_a_pair_scan_equal_record_lines_of_the_host_text(gpu_device, final_newline):
    """The paired text of test_text_stream_equals_the_one_shot_scan (700 pairs, R2's names longer than R1's, R2 three
    records longer): every name equals ``record_lines`` on the host text for that record and side."""
    from genefuserust_amd.fastq import fastq_cut_device, record_lines
    from genefuserust_amd.hit_names import hit_names_device
    from genefuserust_amd.read_pair import scan_pairs_device
    ix, genes = _golden_index()
    rng = np.random.default_rng(3)
    pairs = _make_pairs(rng, genes, 700)
    t1 = b"\n".join(b"@p%d/1\n%s\n+\n%s" % (k, p[0], p[1]) for k, p in enumerate(pairs))
    extra = pairs + pairs[:3]
    t2 = b"\n".join(b"@pair_with_a_longer_name_%d/2\n%s\n+\n%s" % (k, p[2], p[3]) for k, p in enumerate(extra))
    if final_newline:
        t1, t2 = t1 + b"\n", t2 + b"\n"
    d1, d2 = _device_text(t1), _device_text(t2)
    b1, b2 = fastq_cut_device(ix, d1), fastq_cut_device(ix, d2)
    o2 = b2.offsets[:701]
    base = 1_000_000_007
    scan = scan_pairs_device(ix, b1.bases, b1.quals, b1.offsets, b2.bases[:int(o2[-1])], b2.quals[:int(o2[-1])], o2, 150,
                             pair_id_base=base, hits_cap=2100, bytes_cap=700_000)
    nm = hit_names_device(ix, scan, d1, b1, d2, b2, pair_id_base=base)
    names = nm.download()
    rec = scan.download()[0]
    assert len(names) == rec.shape[0] > 100
    assert {int(s) for s in rec["source"]} == {0, 1, 2}
    for h, name in zip(rec, names):
        i = int(h["pair_id"]) - base
        want = record_lines(b2, t2, i)[0] if int(h["source"]) == 2 else record_lines(b1, t1, i)[0]
        assert name == want, (i, int(h["source"]))
        assert name == (b"@pair_with_a_longer_name_%d/2" % i if int(h["source"]) == 2 else b"@p%d/1" % i)
    tot = nm.totals.cpu().numpy()
    assert int(tot[0]) == len(names) and int(tot[1]) == sum(len(x) for x in names) and int(tot[2]) == 0 == int(tot[3])
    off = nm.offsets[:len(names) + 1].cpu().numpy()
    assert off[0] == 0 and (np.diff(off) == [len(x) for x in names]).all()
    ix.close()


def _records(ids_and_sources):
    """gf_pair_hit records that name the given (FASTQ record, source) pairs, and the totals of a scan that found them."""
    import torch
    from genefuserust_amd import _lib
    rec = np.zeros(len(ids_and_sources), dtype=_lib.PAIR_HIT_DTYPE)
    for k, (i, s) in enumerate(ids_and_sources):
        rec[k]["pair_id"], rec[k]["source"] = i, s
    hits = torch.from_numpy(rec.view(np.uint8).reshape(-1, 64).copy() if len(rec) else np.zeros((0, 64), np.uint8))
    totals = torch.zeros(8, dtype=torch.int64)
    totals[0] = len(rec)
    return hits, totals


def _scan_of(ids_and_sources, cap=None, base=0):
    import torch
    from genefuserust_amd.read_pair import PairScan
    ids = [(i + base, s) for i, s in ids_and_sources]
    hits, totals = _records(ids)
    room = torch.zeros((max(cap or len(ids), 1), 64), dtype=torch.uint8)
    room[:hits.shape[0]] = hits
    e = torch.zeros(1, dtype=torch.uint8, device="cuda")
    return PairScan(room.cuda(), e, e, totals.cuda())


@pytest.mark.gpu
def test_names_first_record_last_line_zero_records_and_records_off_the_text(gpu_device):
    from genefuserust_amd.fastq import fastq_cut_device, record_lines
    from genefuserust_amd.hit_names import hit_names_device
    ix, _ = _golden_index()
    # R1 ends in a name line without a newline (a trailing group of one line: no record, but a line to cut);
    # R2 has a '\r' in a name and an empty name line
    t1 = b"@first read/1\nACGT\n+\nFFFF\n@second/1 x\nAC\n+\nFF\n@third/1\n\n+\n\n@a_name_and_nothing_else"
    t2 = b"@first read/2\r\nTTTT\n+\nFFFF\n\nAC\n+\nFF\n@third_of_R2_with_a_long_name_" + b"z" * 300 + b"\nA\n+\nF"
    d1, d2 = _device_text(t1), _device_text(t2)
    b1, b2 = fastq_cut_device(ix, d1), fastq_cut_device(ix, d2)
    assert b1.n_records == 3 and b1.n_newlines == 12 and b2.n_records == 3 and b2.n_newlines == 11
    ids = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 2), (2, 1), (3, 1)]
    base = 5_000_000_000
    scan = _scan_of(ids, cap=16, base=base)
    nm = hit_names_device(ix, scan, d1, b1, d2, b2, pair_id_base=base, names_cap=1000)
    names = nm.download()
    # (record_lines cuts all four lines of a record: the lone last line of R1 is written out here)
    want = [record_lines(b2 if s == 2 else b1, t2 if s == 2 else t1, i)[0] for i, s in ids[:-1]]
    want.append(b"@a_name_and_nothing_else")
    assert want == [b"@first read/1", b"@first read/2\r", b"@second/1 x", b"",
                    b"@third_of_R2_with_a_long_name_" + b"z" * 300, b"@third/1", b"@a_name_and_nothing_else"]
    assert names == want
    assert [int(x) for x in nm.totals.cpu()] == [7, sum(len(x) for x in want), 0, 0]
    # single-end input: no second text — a record of source 2 has no name line; so has one beyond the text's lines,
    # and one before pair_id_base
    scan = _scan_of([(0, 1), (1, 2), (4, 1), (-1, 1), (2, 0)], base=base)
    nm = hit_names_device(ix, scan, d1, b1, pair_id_base=base)
    assert nm.download() == [b"@first read/1", b"", b"", b"", b"@third/1"]
    assert [int(x) for x in nm.totals.cpu()] == [5, 21, 0, 3]
    # zero records (a capacity, but totals[0] == 0), and more records than the capacity
    nm = hit_names_device(ix, _scan_of([], cap=8), d1, b1, d2, b2)
    assert nm.download() == [] and [int(x) for x in nm.totals.cpu()] == [0, 0, 0, 0]
    assert int(nm.offsets[0].item()) == 0
    scan = _scan_of([(0, 1), (1, 1), (2, 1)])
    scan.totals[0] = 1000   # (the scan found more than it had room for)
    assert hit_names_device(ix, scan, d1, b1).download() == [b"@first read/1", b"@second/1 x", b"@third/1"]
    ix.close()


@pytest.mark.gpu
def test_names_capacity_one_byte_too_small(gpu_device):
    """The overflow bit, the bytes needed, every name that fits where it belongs, and nothing past the capacity."""
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.hit_names import HitNames, hit_names_device, lib
    ix, _ = _golden_index()
    want = [b"@read_number_%d_of_the_file" % k for k in range(300)]
    t1 = b"".join(n + b"\nACGT\n+\nFFFF\n" for n in want)
    d1 = _device_text(t1)
    b1 = fastq_cut_device(ix, d1)
    ids = [(k, 1) for k in range(0, 300, 2)]
    want = [want[k] for k, _ in ids]
    need = sum(len(x) for x in want)
    scan = _scan_of(ids)
    cap = need - 1
    guard = 4096
    names = torch.full((cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    off = torch.zeros(len(ids) + 1, dtype=torch.int64, device="cuda")
    tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    L = lib()
    ws_bytes = int(L.gf_hn_workspace_bytes(len(ids)))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc_ = L.gf_hn_names_device(ix._handle(), scan.hits.data_ptr(), scan.totals.data_ptr(), len(ids), 0, d1.data_ptr(),
                               d1.numel(), b1.nl_pos.data_ptr(), b1.n_newlines, None, 0, None, 0, ws.data_ptr(), ws_bytes,
                               names.data_ptr(), cap, off.data_ptr(), tot.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
    assert rc_ == _lib.GF_OK
    torch.cuda.synchronize()
    assert [int(x) for x in tot.cpu()] == [len(ids), need, 1, 0]
    o = off.cpu().numpy()
    assert (np.diff(o) == [len(x) for x in want]).all() and o[-1] == need   # the offsets are the true ones
    got = names.cpu().numpy().tobytes()
    assert got[:o[-2]] == b"".join(want[:-1])                 # every name that fits
    assert got[o[-2]:] == b"\xa5" * (len(got) - o[-2])         # the last one is not started, the guard untouched
    with pytest.raises(_lib.GfError) as e:
        HitNames(names[:cap], off, tot).download()
    assert e.value.code == _lib.GF_ERR_CAPACITY
    # with the bytes it asked for
    assert hit_names_device(ix, scan, d1, b1, names_cap=need).download() == want
    ix.close()


# ---- 2. the single-end stream against the one-shot scan and the oracle ------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes,final_newline", [(7_000, False), (40_000, True), (10_000_000, False)])
def test_single_end_stream_equals_the_one_shot_scan(gpu_device, oracle, chunk_bytes, final_newline):
    import torch
    from genefuserust_amd import Indexer
    from genefuserust_amd.scan_stream import scan_single_text_stream
    from genefuserust_amd.single_end import scan_single_device
    from genefuserust_amd.synth import ragged_batch
    genes, rev, reads = _synthetic(n_reads=4000)
    n = len(reads)
    quals = _quals_for(reads, 9)
    ix = Indexer.from_gene_slices(genes, rev)
    ix.make_index()
    text = b"\n".join(b"@read %d of the run\n%s\n+\n%s" % (k, r, q) for k, (r, q) in enumerate(zip(reads, quals)))
    if final_newline:
        text += b"\n"
    assert len(text) < chunk_bytes or len(text) > 10 * chunk_bytes
    got = list(scan_single_text_stream(ix, np.frombuffer(text, dtype=np.uint8).copy(), chunk_bytes=chunk_bytes,
                                       max_read_len=300))
    assert sum(t[4]["reads"] for t in got) == n
    assert len(got) >= (10 if chunk_bytes < len(text) else 1)
    # the one-shot scan of the whole batch
    b, off = ragged_batch(reads)
    q, _ = ragged_batch(quals)
    dev = [torch.from_numpy(a).cuda() for a in (b, q, off)]
    want = scan_single_device(ix, *dev, 300, hits_cap=n, bytes_cap=int(b.size) + 64, retry_cap=n).download()
    assert want[3]["overflow"] == 0 and want[3]["hits"] > 0 and want[3]["retried_reads"] > 0
    rec = np.concatenate([t[0] for t in got])
    assert rec.shape[0] == want[0].shape[0] == want[3]["hits"]
    for f in ("pair_id", "source", "flags", "read_len", "merge_diff"):
        assert (rec[f] == want[0][f]).all(), f
    assert rec["m"].tobytes() == want[0]["m"].tobytes()
    k = 0
    for r, hb, hq, names, tot in got:   # the reads and the names travel with their records (offsets are per chunk)
        assert len(names) == r.shape[0] == tot["hits"] and tot["overflow"] == 0
        for h, name in zip(r, names):
            o, ln = int(h["seq_offset"]), int(h["read_len"])
            w = want[0][k]
            wo = int(w["seq_offset"])
            assert hb[o:o + ln] == want[1][wo:wo + ln] and hq[o:o + ln] == want[2][wo:wo + ln]
            assert name == b"@read %d of the run" % int(h["pair_id"])
            k += 1
    for f in ("hits", "hit_bytes", "retried_reads"):
        assert sum(t[4][f] for t in got) == want[3][f], f
    # the same hits from the oracle's map_read and the direction rule, read by read
    ox = oracle.OracleIndexer(genes)
    exp = []
    for i, read in enumerate(reads):
        mp = [tuple(m) for m in ox.map_read(read)]
        if len(mp) != 2:
            continue
        if oracle.in_required_direction(mp, rev):
            exp.append((i, 0, read, quals[i], mp))
            continue
        rr = oracle.reverse_complement(read)
        mp = [tuple(m) for m in ox.map_read(rr)]
        if len(mp) == 2 and oracle.in_required_direction(mp, rev):
            exp.append((i, 3, rr, quals[i][::-1], mp))
    assert sum(1 for e in exp if e[1] == 0) > 0 and sum(1 for e in exp if e[1] == 3) > 0
    assert len(exp) == rec.shape[0]
    k = 0
    for r, hb, hq, names, tot in got:
        for h in r:
            i, flags, seq, qual, mp = exp[k]
            o, ln = int(h["seq_offset"]), int(h["read_len"])
            assert (int(h["pair_id"]), int(h["flags"]), hb[o:o + ln], hq[o:o + ln]) == (i, flags, seq, qual)
            assert [(int(h["m"][j]["seq_start"]), int(h["m"][j]["seq_end"]), int(h["m"][j]["contig"]),
                     int(h["m"][j]["position"])) for j in range(2)] == mp
            k += 1
    ix.close()


# ---- 3. files -------------------------------------------------------------------------------------------------------

def _names_of(results):
    return [(m.m_name, m.m_read, m.m_quality, m.m_reversed) for fr in results for m in fr.m_matches]


def _same_scan(streamed, whole, count_key, n):
    (s_res, s_cnt), (w_res, w_cnt) = streamed, whole
    s_cnt = dict(s_cnt)
    assert s_cnt.pop("chunks") >= 3 and "chunks" not in w_cnt
    assert s_cnt == w_cnt and w_cnt[count_key] == n
    assert _texts(s_res) == _texts(w_res) and _names_of(s_res) == _names_of(w_res)
    assert w_cnt["fusions"] >= 1 and len(w_res) >= 1 and len(_names_of(w_res)) >= 1


def _gz(path):
    out = path + ".gz"
    with gzip.open(out, "wb") as f:
        f.write(open(path, "rb").read())
    return out


@pytest.mark.gpu
def test_pair_end_files_in_chunks_equal_the_whole_file_route(gpu_device, tmp_path):
    from genefuserust_amd.multi_csv_scan import scan_report
    from genefuserust_amd.scan import scan_pair_end_report
    fa, lst, csvs, r1, r2 = _files(tmp_path)
    c = 12_000
    assert os.path.getsize(r1) > 3 * c and os.path.getsize(r2) > 3 * c
    for csv in (csvs[0], csvs[1], csvs[3]):   # GA|GB, GA|GR (a gene on the reverse strand), all four genes
        whole = scan_pair_end_report(fa, csv, r1, r2)
        _same_scan(scan_pair_end_report(fa, csv, r1, r2, chunk_bytes=c), whole, "pairs", 150)
    # gzipped, and a chunk that holds everything
    z1, z2 = _gz(r1), _gz(r2)
    whole = scan_pair_end_report(fa, csvs[3], r1, r2)
    _same_scan(scan_pair_end_report(fa, csvs[3], z1, z2, chunk_bytes=c), whole, "pairs", 150)
    one = scan_pair_end_report(fa, csvs[3], z1, r2, chunk_bytes=1 << 20)
    assert one[1]["chunks"] == 1 and _texts(one[0]) == _texts(whole[0])
    assert any(m.m_source == "merged" and b" merged_diff_" in m.m_name for fr in whole[0] for m in fr.m_matches)
    # the mode switch passes the option through
    _same_scan(scan_report(fa, csvs[0], r1, r2, chunk_bytes=c), scan_pair_end_report(fa, csvs[0], r1, r2), "pairs", 150)
    _same_scan(scan_report(fa, csvs[1], r1, chunk_bytes=c), scan_report(fa, csvs[1], r1), "reads", 150)
    with pytest.raises(ValueError, match="chunk_bytes"):
        scan_report(fa, lst, r1, r2, chunk_bytes=c)


@pytest.mark.gpu
def test_single_end_files_in_chunks_equal_the_whole_file_route(gpu_device, tmp_path):
    """The planted fusion of test_files_device_route_equals_host_route_on_gzipped_planted_fusion, plain and gzipped."""
    from genefuserust_amd.scan import scan_single_end_report
    rng = np.random.default_rng(31)
    chrs = {"chr1": rand_seq(rng, 9000), "chr2": rand_seq(rng, 8000)}
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b"".join(b">" + k.encode() + b"\n" + v + b"\n" for k, v in chrs.items()))
    csv = tmp_path / "f.csv"
    csv.write_text(">GA,chr1:1000-8000\n1,1000,4000\n2,5000,8000\n\n>GB,chr2:500-7500\n1,500,3000\n2,4000,7500\n")
    ga, gb = chrs["chr1"][999:8000], chrs["chr2"][499:7500]
    p, q = 3000, 2500
    junction = ga[p - 400:p] + gb[q:q + 400]
    recs = []
    for k in range(120):
        if k % 3 == 2:
            s = rand_seq(rng, 150)
        else:
            o = int(rng.integers(290, 360))
            s = junction[o:o + 150]
            if k % 2:
                s = rc(s)       # read off the other strand
            if k % 7 == 0:
                s = s.lower()
        qual = bytes(rng.integers(35, 74, size=len(s), dtype=np.uint8))
        recs += [b"@read%d/1" % k, s, b"+", qual]
    plain = tmp_path / "R1.fq"
    plain.write_bytes(b"\n".join(recs))   # (no final newline)
    zipped = tmp_path / "R1.fq.gz"
    with gzip.open(zipped, "wb") as f:
        f.write(b"\n".join(recs) + b"\n")
    c = 9_000
    assert os.path.getsize(plain) > 3 * c
    whole = scan_single_end_report(str(fa), str(csv), str(plain))
    for fq in (plain, zipped):
        _same_scan(scan_single_end_report(str(fa), str(csv), str(fq), chunk_bytes=c), whole, "reads", 120)
    ms = [m for fr in whole[0] for m in fr.m_matches]
    assert any(m.m_reversed for m in ms) and any(not m.m_reversed for m in ms)
    with pytest.raises(ValueError, match="chunk_bytes"):
        scan_single_end_report(str(fa), str(csv), str(plain), route="host", chunk_bytes=c)


@pytest.mark.gpu
def test_a_record_that_does_not_fit_names_the_file(gpu_device, tmp_path):
    from genefuserust_amd import _lib
    from genefuserust_amd.scan import scan_single_end_report
    fa, lst, csvs, r1, r2 = _files(tmp_path)
    bad = tmp_path / "long_line.fq"
    bad.write_bytes(b"@r0\nACGT\n+\nFFFF\n@r1\n" + b"A" * (3 << 20) + b"\n+\n" + b"F" * (3 << 20) + b"\n")
    with pytest.raises(_lib.GfError) as e:
        scan_single_end_report(fa, csvs[0], str(bad), chunk_bytes=4096)
    assert e.value.code == _lib.GF_ERR_CAPACITY and "long_line.fq" in str(e.value)


# ---- 4. bounded memory ------------------------------------------------------------------------------------------------

def _big_fastq(tmp_path, n_pairs):
    """R1 / R2 of ``n_pairs`` pairs of 150 bases (a planted junction every 40th pair), once and four times over."""
    fa, lst, csvs, _, _ = _files(tmp_path)
    rng = np.random.default_rng(12)
    chr1, chr2 = (open(fa, "rb").read().split(b"\n")[k] for k in (1, 3))
    ga, gb = chr1[1000:7000], chr2[500:6500]
    junction = ga[2300 - 300:2300] + gb[3100:3100 + 300]
    l_txt, r_txt = [], []
    for k in range(n_pairs):
        if k % 40 == 0:
            lo = int(rng.integers(90, 230))
            f = junction[lo:lo + int(rng.integers(190, 290))]
        else:
            f = rand_seq(rng, 280)
        s1, s2 = f[:150], rc(f)[:150]
        l_txt.append(b"@pair%06d/1\n%s\n+\n%s\n" % (k, s1, b"F" * len(s1)))
        r_txt.append(b"@pair%06d/2\n%s\n+\n%s\n" % (k, s2, b"F" * len(s2)))
    paths = {}
    for name, txt in (("R1", b"".join(l_txt)), ("R2", b"".join(r_txt))):
        for times in (1, 4):
            p = tmp_path / ("%s_x%d.fq" % (name, times))
            p.write_bytes(txt * times)
            paths[(name, times)] = str(p)
    return fa, csvs[0], paths


def _peak(fn):
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["paired", "single"])
def test_streamed_scan_holds_chunks_not_files(gpu_device, tmp_path, layout):
    """The device memory of a streamed scan does not grow with the file: four times the FASTQ (three times as many
    chunks more) adds less than one chunk to the peak, and the peak stays below the whole-file route's."""
    from genefuserust_amd.scan import scan_pair_end_report, scan_single_end_report
    c = 1 << 20
    fa, csv, paths = _big_fastq(tmp_path, 11_000)
    assert os.path.getsize(paths[("R1", 1)]) > 3 * c and os.path.getsize(paths[("R1", 4)]) > 12 * c

    def run(times, chunk_bytes):
        if layout == "paired":
            return scan_pair_end_report(fa, csv, paths[("R1", times)], paths[("R2", times)], chunk_bytes=chunk_bytes)
        return scan_single_end_report(fa, csv, paths[("R1", times)], chunk_bytes=chunk_bytes)
    run(1, c)   # (warm: what the first call of a process allocates once is in neither figure)
    (res1, cnt1), short = _peak(lambda: run(1, c))
    (res4, cnt4), long_ = _peak(lambda: run(4, c))
    (resw, cntw), whole = _peak(lambda: run(4, None))
    print("peak bytes: streamed short %d, streamed long %d, whole-file long %d; chunks %d / %d"
          % (short, long_, whole, cnt1["chunks"], cnt4["chunks"]))
    assert cnt1["chunks"] >= 3 and cnt4["chunks"] >= 12
    key = "pairs" if layout == "paired" else "reads"
    assert cnt4[key] == 4 * cnt1[key] == 44_000 and cnt4["fusions"] >= 1
    assert _texts(res4) == _texts(resw)
    assert long_ - short < c
    assert long_ < whole


# ---- 5. a byte source that fails ----------------------------------------------------------------------------------------

class _Source:
    """A byte source over a text in memory that does not lend its bytes (they go through the staging blocks);
    ``fail_on``: the number of the ``readinto`` call that raises."""
    name = "<test source>"

    def __init__(self, text: bytes, fail_on: int = 0):
        self.text, self.pos, self.calls, self.fail_on = text, 0, 0, fail_on

    def readinto(self, mv) -> int:
        self.calls += 1
        if self.calls == self.fail_on:
            raise OSError("boom")
        n = min(len(mv), len(self.text) - self.pos)
        mv[:n] = self.text[self.pos:self.pos + n]
        self.pos += n
        return n


def _same_records(chunks, want):
    """The records of a stream's chunks against a one-shot scan's download, the reads with them."""
    rec = np.concatenate([t[0] for t in chunks])
    assert rec.shape[0] == want[0].shape[0] == want[3]["hits"] > 0 and want[3]["overflow"] == 0   # (not vacuous)
    for f in ("pair_id", "source", "flags", "read_len", "merge_diff"):
        assert (rec[f] == want[0][f]).all(), f
    assert rec["m"].tobytes() == want[0]["m"].tobytes()
    k = 0
    for t in chunks:
        for h in t[0]:
            o, ln, wo = int(h["seq_offset"]), int(h["read_len"]), int(want[0][k]["seq_offset"])
            assert t[1][o:o + ln] == want[1][wo:wo + ln] and t[2][o:o + ln] == want[2][wo:wo + ln]
            k += 1


@pytest.mark.gpu
def test_a_single_end_source_that_raises_reaches_the_consumer(gpu_device):
    """The second ``readinto`` of the source raises on an upload thread: the iterator raises it, and the next scan on
    the same index is the one-shot scan's."""
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.scan_stream import scan_single_text_stream
    from genefuserust_amd.single_end import scan_single_device
    ix, genes = _golden_index()
    pairs = _make_pairs(np.random.default_rng(8), genes, 300)
    text = b"".join(b"@read%d\n%s\n+\n%s\n" % (k, p[0], p[1]) for k, p in enumerate(pairs))
    assert len(text) > 10 * 4096
    with pytest.raises(OSError, match="boom"):
        list(scan_single_text_stream(ix, _Source(text, fail_on=2), chunk_bytes=4096, max_read_len=150))
    got = list(scan_single_text_stream(ix, _Source(text), chunk_bytes=4096, max_read_len=150))
    assert sum(t[4]["reads"] for t in got) == 300 and len(got) >= 10
    b = fastq_cut_device(ix, _device_text(text))
    want = scan_single_device(ix, b.bases, b.quals, b.offsets, 150, hits_cap=300, bytes_cap=len(text), retry_cap=300)
    _same_records(got, want.download())
    assert [n for t in got for n in t[3]] == [b"@read%d" % int(i) for t in got for i in t[0]["pair_id"]]
    ix.close()


@pytest.mark.gpu
def test_a_second_file_that_raises_reaches_the_consumer(gpu_device):
    """The same with pairs in which only R2's source raises: on the reader thread of the further side."""
    from genefuserust_amd.fastq import fastq_cut_device
    from genefuserust_amd.read_pair import scan_pairs_device
    from genefuserust_amd.scan_stream import scan_pair_source_stream
    ix, genes = _golden_index()
    pairs = _make_pairs(np.random.default_rng(9), genes, 300)
    t1 = b"".join(b"@pair%d/1\n%s\n+\n%s\n" % (k, p[0], p[1]) for k, p in enumerate(pairs))
    t2 = b"".join(b"@pair%d/2\n%s\n+\n%s\n" % (k, p[2], p[3]) for k, p in enumerate(pairs))
    assert len(t2) > 10 * 4096
    with pytest.raises(OSError, match="boom"):
        list(scan_pair_source_stream(ix, _Source(t1), _Source(t2, fail_on=2), chunk_bytes=4096, max_read_len=150))
    got = list(scan_pair_source_stream(ix, _Source(t1), _Source(t2), chunk_bytes=4096, max_read_len=150))
    assert sum(t[4]["pairs"] for t in got) == 300 and len(got) >= 10
    b1, b2 = fastq_cut_device(ix, _device_text(t1)), fastq_cut_device(ix, _device_text(t2))
    want = scan_pairs_device(ix, b1.bases, b1.quals, b1.offsets, b2.bases, b2.quals, b2.offsets, 150, hits_cap=900,
                             bytes_cap=2 * (len(t1) + len(t2)), retry_cap=900)
    _same_records(got, want.download())
    ix.close()
