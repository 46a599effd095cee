"""Multi-CSV mode with streamed FASTQ files (``scan_multi_csv_report(chunk_bytes=...)``): one pass over the files for
all CSVs of the list, each chunk handed back in one block (scan_pack.py) — against the resident multi-CSV route and
the single-CSV streamed scanners, entry by entry; its read-backs per chunk, its memory, its errors."""
import os

import pytest

from tests.test_multi_csv_scan import _files, _texts
from tests.test_stream_files import _Source, _big_fastq, _gz, _peak


def _entries(got):
    return [(csv, _texts(results), counters) for csv, results, counters in got]


def _without_chunks(got):
    out = []
    for csv, texts, counters in _entries(got):
        counters = dict(counters)
        assert counters.pop("chunks") >= 1
        out.append((csv, texts, counters))
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory, gpu_device):
    """The files of tests/test_multi_csv_scan.py and what the resident route makes of them, paired and single-end:
    computed once, and left as they are."""
    tmp = tmp_path_factory.mktemp("multi_csv_stream")
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    fa, lst, csvs, r1, r2 = _files(tmp)
    resident = scan_multi_csv_report(fa, lst, r1, r2)
    resident_se = scan_multi_csv_report(fa, lst, r1)
    # the floors of the file-level test, so that agreement on nothing cannot pass
    for got in (resident, resident_se):
        with_fusions = [g for g in got[:5] if g[2]["fusions"] >= 1]
        assert len(with_fusions) >= 2 and len({_texts(g[1])[0] for g in with_fusions}) >= 2
        assert got[2][2]["fusions"] == 0 and got[2][1] == []
    return tmp, fa, lst, csvs, r1, r2, _entries(resident), _entries(resident_se)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", [7_000, 40_000, 10_000_000])
def test_pairs_equal_the_resident_route_and_the_single_csv_streamed_scans(files, chunk_bytes):
    from genefuserust_amd.multi_csv_scan import report_names, scan_multi_csv_report
    from genefuserust_amd.scan import scan_pair_end_report
    tmp, fa, lst, csvs, r1, r2, resident, _ = files
    out = tmp / ("out_%d" % chunk_bytes)
    out.mkdir()
    jf = str(out / "rep.json")
    got = scan_multi_csv_report(fa, lst, r1, r2, json_file=jf, command="cmd", version="0.8.0", time="t",
                                chunk_bytes=chunk_bytes)
    assert [g[0] for g in got] == csvs and len(got) == 6
    assert _without_chunks(got) == resident
    alone = {}
    for csv, results, counters in got:
        if csv not in alone:
            alone[csv] = scan_pair_end_report(fa, csv, r1, r2, chunk_bytes=chunk_bytes)
        assert counters == alone[csv][1] and list(counters) == list(alone[csv][1])     # the keys' order too
        assert _texts(results) == _texts(alone[csv][0])
        assert counters["pairs"] == 150 and counters["chunks"] == (1 if chunk_bytes > 1_000_000 else counters["chunks"])
    assert got[0][2]["chunks"] >= (3 if chunk_bytes == 7_000 else 1)
    names = report_names(jf, csvs)
    assert names[0] == names[5] and len(set(names)) == 5
    for name, (_, results, _) in zip(names, got):
        assert open(name).read() == _texts(results)[1]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk_bytes", [7_000, 40_000, 10_000_000])
def test_single_end_equals_the_resident_route_and_the_single_csv_streamed_scans(files, chunk_bytes):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    from genefuserust_amd.scan import scan_single_end_report
    tmp, fa, lst, csvs, r1, r2, _, resident_se = files
    got = scan_multi_csv_report(fa, lst, r1, chunk_bytes=chunk_bytes)
    assert [g[0] for g in got] == csvs
    assert _without_chunks(got) == resident_se
    alone = {}
    for csv, results, counters in got:
        if csv not in alone:
            alone[csv] = scan_single_end_report(fa, csv, r1, chunk_bytes=chunk_bytes)
        assert counters == alone[csv][1] and list(counters) == list(alone[csv][1])
        assert _texts(results) == _texts(alone[csv][0]) and counters["reads"] == 150


@pytest.mark.gpu
def test_gzipped_inputs_and_a_streamed_reference(files):
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    tmp, fa, lst, csvs, r1, r2, resident, resident_se = files
    z1, z2 = _gz(r1), _gz(r2)
    assert _without_chunks(scan_multi_csv_report(fa, lst, z1, z2, chunk_bytes=12_000)) == resident
    assert _without_chunks(scan_multi_csv_report(fa, lst, z1, r2, chunk_bytes=12_000, ref_chunk_bytes=7)) == resident
    assert _without_chunks(scan_multi_csv_report(fa, lst, z1, chunk_bytes=12_000, ref_chunk_bytes=7)) == resident_se


@pytest.mark.gpu
def test_two_read_backs_per_chunk_and_only_the_overflowed_csv_is_scanned_again(files, monkeypatch):
    from genefuserust_amd import scan_pack, scan_stream
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    tmp, fa, lst, csvs, r1, r2, resident, _ = files
    copies, alone = [], []
    to_host, scan_alone = scan_pack._to_host, scan_stream._scan_alone
    monkeypatch.setattr(scan_pack, "_to_host", lambda t: (copies.append(t.numel()), to_host(t))[1])

    def counted(step, first_caps, *rest):
        alone.append(first_caps)
        return scan_alone(step, first_caps, *rest)
    monkeypatch.setattr(scan_stream, "_scan_alone", counted)
    got = scan_multi_csv_report(fa, lst, r1, r2, chunk_bytes=12_000)
    chunks = got[0][2]["chunks"]
    assert chunks >= 3 and _without_chunks(got) == resident
    # K = 6: the headers and the body of one block per chunk, and no scan with a read-back of its own
    assert len(copies) == 2 * chunks and copies[0::2] == [64 * 7] * chunks and alone == []
    # a record capacity of 2 per CSV and chunk: the CSVs with more hits in a chunk overflow, the one without hits
    # (GB + GC, nothing planted) never does; the entries are the same
    del copies[:]
    got = scan_multi_csv_report(fa, lst, r1, r2, chunk_bytes=12_000, hits_cap=2)
    assert _without_chunks(got) == resident
    assert len(copies) == 2 * chunks
    hits_per_entry = [c["matches_before_filtering"] for _, _, c in got]
    assert hits_per_entry[2] == 0 and min(hits_per_entry[:2]) > 2 * chunks
    # at least one rescan per chunk for the entries with that many hits, none for the empty one: fewer than K a chunk
    assert 2 * chunks <= len(alone) <= 5 * chunks
    assert all(caps["hits_cap"] > 2 and caps["retry_cap"] > 0 for caps in alone)


@pytest.mark.gpu
def test_streamed_multi_csv_holds_chunks_not_files(gpu_device, tmp_path):
    """As tests/test_stream_files.py::test_streamed_scan_holds_chunks_not_files: with the file four times as large the
    device's peak does not depend on the file size, and the host's peak grows by less than one chunk.  The host holds
    the staging blocks and the matches; the matches grow with the file whatever the route, so the host's figure is
    taken with two panels that match nothing (GB + GC), the device's with one that finds the planted fusion."""
    import tracemalloc
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report
    c = 1 << 20
    fa, csv, paths = _big_fastq(tmp_path, 11_000)
    none = str(tmp_path / "none.csv")
    assert os.path.isfile(none)
    lst, lst_none = tmp_path / "two.txt", tmp_path / "none_twice.txt"
    lst.write_text("%s\n%s\n" % (csv, none))
    lst_none.write_text("%s\n%s\n" % (none, none))

    def run(times, panels=lst):
        return scan_multi_csv_report(fa, str(panels), paths[("R1", times)], paths[("R2", times)], chunk_bytes=c)

    def host_peak(times):
        tracemalloc.start()
        got = run(times, lst_none)
        peak = tracemalloc.get_traced_memory()[1]
        tracemalloc.stop()
        assert [g[2]["matches_before_filtering"] for g in got] == [0, 0] and got[0][2]["pairs"] == 11_000 * times
        return peak
    run(1)   # (warm: what the first call of a process allocates once is in neither figure)
    got1, dev1 = _peak(lambda: run(1))
    got4, dev4 = _peak(lambda: run(4))
    host1, host4 = host_peak(1), host_peak(4)
    print("peaks: device %d / %d, host %d / %d; chunks %d / %d" % (dev1, dev4, host1, host4, got1[0][2]["chunks"],
                                                                   got4[0][2]["chunks"]))
    assert got1[0][2]["chunks"] >= 3 and got4[0][2]["chunks"] >= 12
    assert got4[0][2]["pairs"] == 4 * got1[0][2]["pairs"] == 44_000
    assert got4[0][2]["fusions"] >= 1 and got4[1][2]["fusions"] == 0
    assert dev4 - dev1 < c
    assert host4 - host1 < c


@pytest.mark.gpu
def test_a_second_file_that_raises_reaches_the_caller_and_every_index_is_closed(files, monkeypatch):
    from genefuserust_amd import Indexer
    from genefuserust_amd.fastq import FastqReader
    from genefuserust_amd.multi_csv_scan import scan_multi_csv_report, scan_report
    tmp, fa, lst, csvs, r1, r2, resident, _ = files
    made = []
    make_index = Indexer.make_index
    monkeypatch.setattr(Indexer, "make_index", lambda self, *a, **k: (made.append(self), make_index(self, *a, **k))[1])

    class _Failing(_Source):
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass
    open_stream = FastqReader.open_stream
    monkeypatch.setattr(FastqReader, "open_stream", lambda self: _Failing(open(r2, "rb").read(), fail_on=2)
                        if self.m_filename == r2 else open_stream(self))
    with pytest.raises(OSError, match="boom"):
        scan_multi_csv_report(fa, lst, r1, r2, chunk_bytes=4096)
    assert len(made) == 6 and all(ix._h is None for ix in made)
    monkeypatch.undo()
    # and the next run is whole
    assert _without_chunks(scan_multi_csv_report(fa, lst, r1, r2, chunk_bytes=4096)) == resident
    # the mode switch keeps refusing
    with pytest.raises(ValueError, match="chunk_bytes"):
        scan_report(fa, lst, r1, r2, chunk_bytes=4096)
