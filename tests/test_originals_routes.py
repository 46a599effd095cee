"""``originals=True`` on every file-level route: the matches carry the FASTQ records they came from — both mates of a
pair, the one read of single-end input — the same records and the same HTML report whether the files are read whole
or streamed (where ``gf_hn_records_device`` gathers them before a chunk goes), plain or gzipped, one CSV or a list."""
import gzip

import pytest

from tests.test_multi_csv_scan import _files

CHUNK = 12_000   # the FASTQ files are 48 kB: four chunks or more


def _html(results):
    from genefuserust_amd import report_html
    return report_html(results, "cmd", "0.8.0", "t")


def _originals(results):
    return [[m.m_original_reads for m in fr.m_matches] for fr in results]


def _host_records(path):
    lines = open(path, "rb").read().split(b"\n")
    return {lines[k].split(b"/")[0]: tuple(lines[k:k + 4]) for k in range(0, len(lines) - 3, 4)}


def _held_to_the_files(results, *paths):
    """Every match carries the records of its pair (its read), as the lines of the files say."""
    records = [_host_records(p) for p in paths]
    n = 0
    for fr in results:
        for m in fr.m_matches:
            key = m.m_name.split(b"/")[0]
            assert m.m_original_reads == [r[key] for r in records], m.m_name
            assert all(len(rec) == 4 and rec[2] == b"+" for rec in m.m_original_reads)
            n += 1
    assert n > 0
    return n


@pytest.mark.gpu
def test_pairs_streamed_equal_whole_file_plain_and_gzipped(gpu_device, tmp_path):
    from genefuserust_amd.scan import scan_pair_end_files, scan_pair_end_report
    fa, _, csvs, r1, r2 = _files(tmp_path)
    csv = csvs[3]
    whole, counters = scan_pair_end_report(fa, csv, r1, r2, originals=True)
    assert counters["fusions"] >= 1
    _held_to_the_files(whole, r1, r2)
    assert all(len(m.m_original_reads) == 2 for fr in whole for m in fr.m_matches)   # both mates, whichever matched
    page = _html(whole)
    assert "<xmp>@pair" in page and "/2\n" in page[page.index("<xmp>"):page.index("</xmp>")]
    streamed, s_counters = scan_pair_end_report(fa, csv, r1, r2, originals=True, chunk_bytes=CHUNK)
    assert s_counters["chunks"] >= 3 and {k: v for k, v in s_counters.items() if k != "chunks"} == counters
    assert streamed == whole and _originals(streamed) == _originals(whole) and _html(streamed) == page
    # the same from gzipped files, whole and streamed
    z1, z2 = str(tmp_path / "Z1.fq.gz"), str(tmp_path / "Z2.fq.gz")
    for src, dst in ((r1, z1), (r2, z2)):
        with gzip.open(dst, "wb") as f:
            f.write(open(src, "rb").read())
    for kwargs in ({}, dict(chunk_bytes=CHUNK)):
        zipped, _ = scan_pair_end_report(fa, csv, z1, z2, originals=True, **kwargs)
        assert _originals(zipped) == _originals(whole) and _html(zipped) == page, kwargs
    # without originals: the same matches, none of them with records, and another page
    plain, p_counters = scan_pair_end_report(fa, csv, r1, r2, chunk_bytes=CHUNK)
    assert plain == whole and p_counters == s_counters
    assert all(m.m_original_reads == [] for fr in plain for m in fr.m_matches)
    assert "<xmp></xmp>" in _html(plain) and "<xmp></xmp>" not in page
    # the match lists themselves
    kept, _ = scan_pair_end_files(fa, csv, r1, r2, originals=True, chunk_bytes=CHUNK)
    w_kept, _ = scan_pair_end_files(fa, csv, r1, r2, originals=True)
    assert kept == w_kept and [m.m_original_reads for m in kept] == [m.m_original_reads for m in w_kept]
    assert all(len(m.m_original_reads) == 2 for m in kept)


@pytest.mark.gpu
def test_single_end_streamed_host_route_and_whole_file_agree(gpu_device, tmp_path):
    from genefuserust_amd.scan import scan_single_end_report
    fa, _, csvs, r1, _ = _files(tmp_path)
    csv = csvs[3]
    whole, counters = scan_single_end_report(fa, csv, r1, originals=True)
    assert counters["fusions"] >= 1
    _held_to_the_files(whole, r1)
    assert all(len(m.m_original_reads) == 1 for fr in whole for m in fr.m_matches)
    page = _html(whole)
    streamed, s_counters = scan_single_end_report(fa, csv, r1, originals=True, chunk_bytes=CHUNK)
    assert s_counters["chunks"] >= 3
    host, _ = scan_single_end_report(fa, csv, r1, originals=True, route="host")
    z1 = str(tmp_path / "Z1.fq.gz")
    with gzip.open(z1, "wb") as f:
        f.write(open(r1, "rb").read())
    zipped, _ = scan_single_end_report(fa, csv, z1, originals=True, chunk_bytes=CHUNK)
    for other in (streamed, host, zipped):
        assert other == whole and _originals(other) == _originals(whole) and _html(other) == page


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", [None, CHUNK])
def test_multi_csv_equals_the_single_csv_scan_of_each_csv(gpu_device, tmp_path, chunk_bytes):
    from genefuserust_amd.multi_csv_scan import report_names, scan_multi_csv_report
    from genefuserust_amd.scan import scan_pair_end_report, scan_single_end_report
    fa, lst, csvs, r1, r2 = _files(tmp_path)
    hf = str(tmp_path / "rep.html")
    got = scan_multi_csv_report(fa, lst, r1, r2, originals=True, chunk_bytes=chunk_bytes, html_file=hf, command="cmd",
                                version="0.8.0", time="t")
    assert [g[0] for g in got] == csvs
    alone = {}
    for name, (csv, results, _) in zip(report_names(hf, csvs), got):
        if csv not in alone:
            alone[csv] = scan_pair_end_report(fa, csv, r1, r2, originals=True)[0]
        assert results == alone[csv] and _originals(results) == _originals(alone[csv])
        assert open(name, encoding="utf-8").read() == _html(alone[csv])
        if results:
            _held_to_the_files(results, r1, r2)
    assert sum(1 for g in got if g[1]) >= 2
    # single-end, and no file asked for
    se = scan_multi_csv_report(fa, lst, r1, originals=True, chunk_bytes=chunk_bytes)
    for csv, results, _ in se[:2]:
        want = scan_single_end_report(fa, csv, r1, originals=True)[0]
        assert results == want and _originals(results) == _originals(want) and _html(results) == _html(want)
    assert sum(1 for g in se if g[1]) >= 2


@pytest.mark.gpu
def test_the_device_tail_keeps_the_originals(gpu_device, tmp_path):
    from genefuserust_amd.multi_csv_scan import scan_report
    fa, _, csvs, r1, r2 = _files(tmp_path)
    hf, jf = str(tmp_path / "a.html"), str(tmp_path / "a.json")
    host, _ = scan_report(fa, csvs[3], r1, r2, originals=True, chunk_bytes=CHUNK, html_file=hf, json_file=jf,
                          command="cmd", version="0.8.0", time="t")
    dev, _ = scan_report(fa, csvs[3], r1, r2, originals=True, chunk_bytes=CHUNK, tail="device")
    assert dev == host and _originals(dev) == _originals(host) and _html(dev) == _html(host)
    _held_to_the_files(dev, r1, r2)
    assert open(hf, encoding="utf-8").read() == _html(host) and open(jf).read().startswith("{\n\t\"command\":\"cmd\"")
    se_host, _ = scan_report(fa, csvs[3], r1, originals=True)
    se_dev, _ = scan_report(fa, csvs[3], r1, originals=True, tail="device")
    assert _originals(se_dev) == _originals(se_host) and _html(se_dev) == _html(se_host)


@pytest.mark.gpu
def test_without_originals_the_gather_is_never_called(gpu_device, tmp_path, monkeypatch):
    from genefuserust_amd import hit_names
    from genefuserust_amd.scan import scan_pair_end_files
    fa, _, csvs, r1, r2 = _files(tmp_path)
    want, w_counters = scan_pair_end_files(fa, csvs[3], r1, r2, chunk_bytes=CHUNK, originals=True)
    assert any(m.m_original_reads for m in want)

    def boom(*a, **k):
        raise AssertionError("hit_records_device was called without originals")
    monkeypatch.setattr(hit_names, "hit_records_device", boom)
    got, counters = scan_pair_end_files(fa, csvs[3], r1, r2, chunk_bytes=CHUNK)
    assert counters == w_counters and len(got) > 0
    assert got == want                                            # (the records are not part of a match's identity)
    assert all(m.m_original_reads == [] for m in got)
    with pytest.raises(AssertionError, match="without originals"):   # and with them, it is what is called
        scan_pair_end_files(fa, csvs[3], r1, r2, chunk_bytes=CHUNK, originals=True)


@pytest.mark.gpu
def test_a_chunk_whose_records_do_not_fit_is_gathered_once_more(gpu_device, tmp_path, monkeypatch):
    """The first gather of every chunk gets 100 bytes: the streamed loop reads the size it asked for and gathers again."""
    from genefuserust_amd import hit_names
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    from genefuserust_amd.scan import scan_pair_end_files
    fa, lst, csvs, r1, r2 = _files(tmp_path)
    want, _ = scan_pair_end_files(fa, csvs[3], r1, r2, originals=True)
    gather, caps = hit_names.hit_records_device, []

    def tight(*a, **k):
        caps.append(k.get("records_cap"))
        return gather(*a, **dict(k, records_cap=100 if k.get("records_cap") is None else k["records_cap"]))
    monkeypatch.setattr(hit_names, "hit_records_device", tight)
    got, counters = scan_pair_end_files(fa, csvs[3], r1, r2, originals=True, chunk_bytes=CHUNK)
    assert got == want and [m.m_original_reads for m in got] == [m.m_original_reads for m in want]
    retried = [c for c in caps if c is not None]
    assert retried and all(c > 100 for c in retried) and caps.count(None) == counters["chunks"]
    del caps[:]
    multi = scan_multi_csv_report(fa, lst, r1, r2, originals=True, chunk_bytes=CHUNK)
    assert [m.m_original_reads for fr in multi[3][1] for m in fr.m_matches] and any(c is not None for c in caps)
    for fr in multi[3][1]:
        for m in fr.m_matches:
            assert len(m.m_original_reads) == 2 and m.m_original_reads[0][0].startswith(m.m_name.split(b"/")[0])
