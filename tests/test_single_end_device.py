"""The single-end scan on the device (gf_se_scan_device, libgfse.so) against the host policy and the oracle:
golden branch cases finished by both tails, a ragged synthetic batch against FusionMapper.scan_single_end, the
capacities and their overflow bits, and the file-level device route against the host route."""
import gzip
import json
import os

import numpy as np
import pytest

from tests.helpers import rand_seq, rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _quals_for(reads, seed=5):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(33, 75, size=len(r), dtype=np.uint8)) for r in reads]


def _upload(reads, quals):
    import torch
    from genefuserust_amd.synth import ragged_batch
    b, off = ragged_batch(reads)
    q, _ = ragged_batch(quals)
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(b).to(dev), torch.from_numpy(q).to(dev), torch.from_numpy(off).to(dev),
            max([len(r) for r in reads] + [1]))


def _rm_tuple(m):
    return (m.m_read, m.m_read_break, tuple(m.m_left_gp), tuple(m.m_right_gp), m.m_gap, m.m_left_distance,
            m.m_right_distance, m.m_reversed)


def _device_tail(ix, scan):
    """finish_pair_hits_device on the scan's records -> {pair_id: (read_break, gap, ld, rd, lgp, rgp)}"""
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd.read_pair import finish_pair_hits_device
    out, status = finish_pair_hits_device(ix, scan)
    torch.cuda.synchronize()
    k = int(scan.totals[0].item())
    rm = out[:k].cpu().numpy().view(_lib.READMATCH_DTYPE).reshape(-1)
    st = status[:k].cpu().numpy()
    rec = scan.hits[:k].cpu().numpy().view(_lib.PAIR_HIT_DTYPE).reshape(-1)
    res = {}
    for h, r, s in zip(rec, rm, st):
        if s == _lib.GF_RM_MATCH:
            res[int(h["pair_id"])] = (int(r["read_break"]), int(r["gap"]), int(r["left_distance"]),
                                      int(r["right_distance"]), (int(r["left_contig"]), int(r["left_position"])),
                                      (int(r["right_contig"]), int(r["right_position"])))
    return res


@pytest.mark.gpu
def test_golden_branch_cases_both_tails_equal_the_oracle_chain(gpu_device, oracle):
    from genefuserust_amd import FusionMapper, Indexer
    from genefuserust_amd.read_pair import finish_pair_hits
    from genefuserust_amd.single_end import scan_single_device
    g = json.load(open(os.path.join(GOLDEN, "branch_cases.json")))
    genes = [None if x is None else x.encode() for x in g["genes"]]
    ix = Indexer.from_gene_slices(genes, g["reversed"])
    ix.make_index()
    fm = FusionMapper(ix)
    ox = oracle.OracleIndexer(genes)
    reads = [c["read"].encode() for c in g["cases"]]
    quals = _quals_for(reads)
    b, q, off, max_len = _upload(reads, quals)
    scan = scan_single_device(ix, b, q, off, max_len)
    rec, hb, hq, tot = scan.download()
    assert tot["overflow"] == 0
    host = {i: m for i, m in finish_pair_hits(fm, rec, hb, hq)}
    dev = _device_tail(ix, scan)
    n_match = n_retry = 0
    for i, read in enumerate(reads):
        st, rm = oracle.fusion_map_read(ox, g["reversed"], read, ox.map_read(read))
        reversed_ = False
        seq, qual = read, quals[i]
        if st == 1:  # mapable but no match: retry the reverse complement
            n_retry += 1
            seq, qual = rc(read), quals[i][::-1]
            st, rm = oracle.fusion_map_read(ox, g["reversed"], seq, ox.map_read(seq))
            reversed_ = True
        if st != 2:
            assert i not in host and i not in dev
            continue
        n_match += 1
        m = host[i]
        assert m.m_read == seq and m.m_quality == qual and m.m_reversed == reversed_ and m.m_source == "r1"
        want = (rm["read_break"], rm["gap"], rm["left_distance"], rm["right_distance"],
                (rm["left_contig"], rm["left_position"]), (rm["right_contig"], rm["right_position"]))
        assert (m.m_read_break, m.m_gap, m.m_left_distance, m.m_right_distance, tuple(m.m_left_gp),
                tuple(m.m_right_gp)) == want
        assert dev[i] == want
    assert n_match >= 20 and n_retry >= 5 and tot["retried_reads"] == n_retry
    assert len(host) == len(dev) == n_match == tot["hits"]
    ix.close()


def _synthetic(n_reads=200_000, seed=21):
    """Genes (two reversed), reads of 0..300 bases: background, single-gene, junctions between genes read off either
    strand; some lower case, some with N or other IUPAC letters."""
    rng = np.random.default_rng(seed)
    genes = [rand_seq(rng, int(rng.integers(3000, 7000))) for _ in range(6)]
    rev = [False, True, False, False, True, False]
    iupac = np.frombuffer(b"NRYKMSWBDHVN", dtype=np.uint8)
    kinds = rng.random(n_reads)
    lens = rng.integers(0, 301, size=n_reads)
    reads = []
    for i in range(n_reads):
        L = int(lens[i])
        k = kinds[i]
        if k < 0.5 or L < 60:
            r = bytearray(rand_seq(rng, L))
        elif k < 0.75:
            g = genes[int(rng.integers(0, 6))]
            p = int(rng.integers(0, len(g) - L))
            r = bytearray(g[p:p + L])
        else:
            a, c = rng.choice(6, size=2, replace=False)
            ga, gc = genes[int(a)], genes[int(c)]
            brk = int(rng.integers(25, L - 25))
            pa = int(rng.integers(brk, len(ga)))
            pc = int(rng.integers(0, len(gc) - (L - brk)))
            r = bytearray(ga[pa - brk:pa] + gc[pc:pc + L - brk])
        if L and rng.random() < 0.5:
            r = bytearray(rc(bytes(r)))
        u = rng.random()
        if L and u < 0.1:
            r = bytearray(bytes(r).lower())
        elif L and u < 0.2:
            for _ in range(int(rng.integers(1, 4))):
                r[int(rng.integers(0, L))] = int(iupac[int(rng.integers(0, len(iupac)))])
        reads.append(bytes(r))
    return genes, rev, reads


@pytest.fixture(scope="module")
def synth_batch(gpu_device):
    from genefuserust_amd import FusionMapper, Indexer
    genes, rev, reads = _synthetic()
    ix = Indexer.from_gene_slices(genes, rev)
    ix.make_index()
    fm = FusionMapper(ix)
    quals = _quals_for(reads, 9)
    want = fm.scan_single_end(reads)
    yield ix, fm, reads, quals, want
    ix.close()


def _records(fm, scan):
    from genefuserust_amd.read_pair import finish_pair_hits
    rec, hb, hq, tot = scan.download()
    return rec, hb, hq, tot, finish_pair_hits(fm, rec, hb, hq)


@pytest.mark.gpu
def test_ragged_batch_equals_host_scan_single_end(synth_batch):
    from genefuserust_amd.single_end import scan_single_device
    ix, fm, reads, quals, want = synth_batch
    b, q, off, max_len = _upload(reads, quals)
    n = len(reads)
    scan = scan_single_device(ix, b, q, off, max_len, hits_cap=n, bytes_cap=int(b.numel()) + 64, retry_cap=n)
    rec, hb, hq, tot, got = _records(fm, scan)
    assert tot["overflow"] == 0
    exp = [(i, m) for i, m in enumerate(want) if m is not None]
    assert len(exp) >= 1000 and sum(m.m_reversed for _, m in exp) >= 300   # both strands, junctions in numbers
    assert [i for i, _ in got] == [i for i, _ in exp]
    for (i, g), (_, w) in zip(got, exp):
        assert _rm_tuple(g) == _rm_tuple(w), i
        assert g.m_quality == (quals[i][::-1] if w.m_reversed else quals[i])
    assert all(int(f) == (3 if m.m_reversed else 0) for f, (_, m) in zip(rec["flags"], got))
    assert (rec["source"] == 1).all() and (rec["merge_diff"] == 0).all()
    # the default retry slots (gf_se_retry_capacity): this batch retries more reads than that — bit 1, the retry
    # pass emptied, the hits on the reads as they are
    from genefuserust_amd.single_end import lib
    assert tot["retried_reads"] > lib().gf_se_retry_capacity(n)
    rec2, _, _, tot2, got2 = _records(fm, scan_single_device(ix, b, q, off, max_len, hits_cap=n,
                                                             bytes_cap=int(b.numel()) + 64))
    assert tot2["overflow"] == 1 and tot2["retried_reads"] == tot["retried_reads"]
    assert [(i, _rm_tuple(m)) for i, m in got2] == [(i, _rm_tuple(m)) for i, m in got if not m.m_reversed]


@pytest.mark.gpu
def test_capacities_overflow_bits_and_rerun(synth_batch):
    import torch
    from genefuserust_amd import _lib
    from genefuserust_amd.single_end import scan_single_device
    ix, fm, reads, quals, want = synth_batch
    b, q, off, max_len = _upload(reads, quals)
    n = len(reads)
    room = dict(hits_cap=n, bytes_cap=int(b.numel()) + 64, retry_cap=n)
    full_rec, full_hb, full_hq, full_tot, full = _records(fm, scan_single_device(ix, b, q, off, max_len, **room))
    n_fwd = int((full_rec["flags"] == 0).sum())
    assert full_tot["retried_reads"] > 2 and full_tot["hits"] > n_fwd > 10
    # everything far too small: both bits, the true retry count, the hits without the (emptied) retry pass
    scan = scan_single_device(ix, b, q, off, max_len, hits_cap=3, bytes_cap=200, retry_cap=2)
    rec, hb, hq, tot = scan.download()
    assert tot["overflow"] == 3 and tot["retried_reads"] == full_tot["retried_reads"]
    fwd = full_rec[full_rec["flags"] == 0]
    assert tot["hits"] == n_fwd and tot["hit_bytes"] == int(fwd["read_len"].sum())
    assert rec.shape[0] == 3 and (rec["flags"] == 0).all()
    assert list(rec["pair_id"]) == list(fwd["pair_id"][:3])
    assert [tuple(map(tuple, r.tolist())) for r in rec["m"]] == [tuple(map(tuple, r.tolist())) for r in fwd["m"][:3]]
    o = 0
    for h in rec:   # a read's bytes are all there or none: those that fit are exact
        ln = int(h["read_len"])
        assert int(h["seq_offset"]) == o
        if o + ln <= 200:
            i = int(h["pair_id"])
            assert hb[o:o + ln] == reads[i] and hq[o:o + ln] == quals[i]
        o += ln
    # retry room only, outputs too small: bit 2 alone, true totals
    rec, hb, hq, tot = scan_single_device(ix, b, q, off, max_len, hits_cap=5, bytes_cap=300, retry_cap=n).download()
    assert tot["overflow"] == 2 and tot["hits"] == full_tot["hits"] and tot["hit_bytes"] == full_tot["hit_bytes"]
    assert list(rec["pair_id"]) == list(full_rec["pair_id"][:5]) and list(rec["flags"]) == list(full_rec["flags"][:5])
    # output room, retries too many: bit 1 alone
    rec, hb, hq, tot = scan_single_device(ix, b, q, off, max_len, hits_cap=n, bytes_cap=room["bytes_cap"],
                                          retry_cap=1).download()
    assert tot["overflow"] == 1 and tot["hits"] == n_fwd
    # the rerun with room is the result of the roomy call
    rec, hb, hq, tot, got = _records(fm, scan_single_device(ix, b, q, off, max_len, **room))
    assert tot == full_tot and rec.tobytes() == full_rec.tobytes() and hb == full_hb and hq == full_hq
    # read_id_base shifts pair_id and nothing else
    rec5, hb5, _, tot5 = scan_single_device(ix, b, q, off, max_len, read_id_base=1_000_000_007, **room).download()
    assert tot5 == full_tot and hb5 == full_hb
    assert (rec5["pair_id"] == full_rec["pair_id"] + 1_000_000_007).all()
    assert rec5["m"].tobytes() == full_rec["m"].tobytes() and rec5["seq_offset"].tobytes() == full_rec["seq_offset"].tobytes()
    # a non-default stream: the same
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        scan = scan_single_device(ix, b, q, off, max_len, stream=s.cuda_stream, **room)
    s.synchronize()
    rec6, hb6, hq6, tot6 = scan.download()
    assert tot6 == full_tot and rec6.tobytes() == full_rec.tobytes() and hb6 == full_hb and hq6 == full_hq
    # n = 0: zero totals
    e = torch.zeros(16, dtype=torch.uint8, device=b.device)
    z = scan_single_device(ix, e, e, torch.zeros(1, dtype=torch.int64, device=b.device), 150)
    assert (z.totals.cpu().numpy() == 0).all()
    # reads longer than max_read_len: counted, never hits, and the Python call raises
    with pytest.raises(_lib.GfError) as err:
        scan_single_device(ix, b, q, off, 100)
    assert err.value.code == _lib.GF_ERR_READ_TOO_LONG
    lens = np.array([len(r) for r in reads])
    z = scan_single_device(ix, b, q, off, 100, check_lengths=False, **room)
    torch.cuda.synchronize()
    assert int(z.totals[5].item()) == int((lens > 100).sum())
    rec7 = z.download()[0]
    assert (lens[rec7["pair_id"]] <= 100).all()


def _compare_routes(fa, csv, fq):
    from genefuserust_amd.scan import scan_single_end_report
    dev, dc = scan_single_end_report(str(fa), str(csv), str(fq), route="device")
    host, hc = scan_single_end_report(str(fa), str(csv), str(fq), route="host")
    assert "retried_reads" in dc
    dc = dict(dc)
    dc.pop("retried_reads")
    assert dc == hc
    assert dev == host
    return dev, hc


@pytest.mark.gpu
def test_files_device_route_equals_host_route_on_reference_fixtures(gpu_device):
    res, counters = _compare_routes(os.path.join(GOLDEN, "tinyref.fa"), os.path.join(GOLDEN, "fusions.csv"),
                                    os.path.join(GOLDEN, "R1.fq"))
    assert counters["reads"] > 0


@pytest.mark.gpu
def test_files_device_route_equals_host_route_on_gzipped_planted_fusion(gpu_device, tmp_path):
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
    fq = tmp_path / "R1.fq.gz"
    with gzip.open(fq, "wb") as f:
        f.write(b"\n".join(recs) + b"\n")
    res, counters = _compare_routes(fa, csv, fq)
    assert counters["reads"] == 120 and len(res) >= 1
    ms = [m for fr in res for m in fr.m_matches]
    assert any(m.m_reversed for m in ms) and any(not m.m_reversed for m in ms)
