"""The switch of the read QC through the layers, without a GPU: ``need_read_qc``; the keyword on every route that has
``read_filter``, checked before a file is opened; with stubs, every route hands it on only when it is set, the full
FASTQ cut is forced only then, a streamed chunk measures the records the sides share and not the batch, multi-CSV mode
measures once for K indexes; the command line's options down to ``scan_report``; and ``report_json`` of a hand-made
``QcResult`` against the model's."""
import inspect
import json
from contextlib import contextmanager

import numpy as np
import pytest

from genefuserust_amd import multi_csv_scan, read_qc, scan, scan_stream
from genefuserust_amd.read_filter import COUNTER_KEYS, ReadFilter
from genefuserust_amd.read_qc import QcResult, ReadQc, need_read_qc
from tests import read_qc_model as model
from tests.test_scan_pieces import TOT, _Mapper


def test_need_read_qc():
    qc = ReadQc()
    assert need_read_qc(None) is None and need_read_qc(qc) is qc
    assert qc.insert_size is True and ReadQc(insert_size=False).insert_size is False
    for bad in (True, False, "on", 1, {}, ReadQc, "report.json"):
        with pytest.raises(ValueError, match="qc must be None or a ReadQc"):
            need_read_qc(bad)
    for bad in (None, 1, "no"):
        with pytest.raises(ValueError, match="insert_size"):
            ReadQc(insert_size=bad)


def _routes():
    """Every function of the three route modules that takes ``read_filter`` and ``adapter_trim``."""
    out = []
    for module in (scan, scan_stream, multi_csv_scan):
        for name, fn in vars(module).items():
            if inspect.isfunction(fn) and fn.__module__ == module.__name__:
                p = inspect.signature(fn).parameters
                if "read_filter" in p and "adapter_trim" in p:
                    out.append(fn)
    return out


def test_the_keyword_is_keyword_only_on_every_route_that_has_read_filter():
    routes = _routes()
    assert {f.__name__ for f in routes} == {
        "scan_pair_end_files", "scan_pair_end_report", "scan_single_end_files", "scan_single_end_report",
        "streamed_found", "_pair_end_matches", "_single_end_matches", "scan_multi_csv_report", "scan_report",
        "_stream_multi_csv", "scan_pair_source_stream", "scan_single_text_stream", "_scan_source_stream", "_scan_chunk"}
    for fn in routes:
        p = inspect.signature(fn).parameters["qc"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__name__


def test_the_file_level_scans_check_the_keyword_before_any_file_is_opened():
    pair, single = ("no.fa", "no.csv", "r1.fq", "r2.fq"), ("no.fa", "no.csv", "r1.fq")
    for call, files in ((scan.scan_pair_end_files, pair), (scan.scan_pair_end_report, pair),
                        (scan.scan_single_end_files, single), (scan.scan_single_end_report, single),
                        (multi_csv_scan.scan_report, pair), (multi_csv_scan.scan_report, single),
                        (multi_csv_scan.scan_report, ("no.fa", "no.txt", "r1.fq", "r2.fq")),
                        (multi_csv_scan.scan_multi_csv_report, ("no.fa", "no.txt", "r1.fq", "r2.fq"))):
        for bad in ("report.json", True):
            with pytest.raises(ValueError, match="qc must be None or a ReadQc"):
                call(*files, qc=bad)
    for call in (scan_stream.scan_pair_source_stream, scan_stream.scan_single_text_stream):
        with pytest.raises(ValueError, match="qc must be None or a ReadQc"):
            call("ix", *(("r1", "r2") if call is scan_stream.scan_pair_source_stream else ("r1",)), qc=True)


# ---- the routes hand the keyword on only when it is set -----------------------------------------------------------------

class _Qc(ReadQc):
    """A collector that only writes down what it is asked to measure."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def measure(self, indexer, stage, *batches, stream=None):
        self.calls.append((indexer, stage, batches))


class _Indexer:
    m_fusion_seq = ()

    def close(self):
        pass


@contextmanager
def _open_index(*a, **k):
    yield _Indexer(), []


def test_streamed_routes_hand_the_keyword_on_only_when_set(monkeypatch):
    seen = []

    def stream(kind):
        def run(ix, *args, **kw):   # today's signature: whatever is not handed on is not there
            seen.append((kind, kw))
            yield "rec", b"", b"", [], dict(TOT, **{("pairs" if kind == "pair" else "reads"): 10})
        return run
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(scan, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    monkeypatch.setattr(scan_stream, "scan_pair_source_stream", stream("pair"))
    monkeypatch.setattr(scan_stream, "scan_single_text_stream", stream("single"))
    qc = _Qc()
    _, with_qc = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096, qc=qc)
    assert seen[-1] == ("pair", {"max_read_len": None, "qc": qc})
    _, without = scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", chunk_bytes=4096)
    assert seen[-1] == ("pair", {"max_read_len": None})
    assert with_qc == without and list(with_qc) == list(without)   # the counters stay
    scan.scan_single_end_report("ref.fa", "x.csv", "a.fq", chunk_bytes=4096, qc=qc)
    assert seen[-1] == ("single", {"max_read_len": None, "qc": qc})
    scan.scan_single_end_report("ref.fa", "x.csv", "a.fq", chunk_bytes=4096)
    assert seen[-1] == ("single", {"max_read_len": None})


def test_whole_file_routes_measure_around_the_filter(monkeypatch):
    calls = []
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "FusionMapper", lambda ix: _Mapper())

    class _Batch(str):
        def max_read_len(self):
            return 7

    class _Totals:
        def cpu(self):
            return self

        def tolist(self):
            return [0] * 8

    class _Reader:
        def __init__(self, *names):
            self.names = names

        @classmethod
        def from_paths(cls, *names):
            return cls(*names)

        def read_all_device(self, ix):
            pairs = tuple((_Batch("cut " + n), b"text") for n in self.names)
            return pairs if len(pairs) == 2 else pairs[0]

    def filtered(ix, config, *batches):
        calls.append(("filter", batches))
        return tuple(_Batch("kept " + b) for b in batches) + (_Totals(),)

    def found(kind, key):
        def run(*args, **kw):
            calls.append((kind,))
            return [], *scan.route_counters(key, 5, 0, TOT)
        return run
    from genefuserust_amd import read_filter
    monkeypatch.setattr(scan, "FastqReaderPair", _Reader)
    monkeypatch.setattr(scan, "FastqReader", _Reader)
    monkeypatch.setattr(read_filter, "filter_reads_device", filtered)
    monkeypatch.setattr(scan, "pairs_found", found("pairs", "pairs"))
    monkeypatch.setattr(scan, "single_end_found", found("device", "reads"))
    monkeypatch.setattr(scan, "_single_end_host_found", found("host", "reads"))
    qc, cfg = _Qc(), ReadFilter()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, b))
    scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", read_filter=cfg, qc=qc)
    assert calls == [("before", ("cut a.fq", "cut b.fq")), ("filter", ("cut a.fq", "cut b.fq")),
                     ("after", ("kept cut a.fq", "kept cut b.fq")), ("pairs",)]
    del calls[:]
    scan.scan_pair_end_files("ref.fa", "x.csv", "a.fq", "b.fq", qc=qc)   # neither trimming nor filter: no second pass
    assert calls == [("before", ("cut a.fq", "cut b.fq")), ("pairs",)]
    for route in ("device", "host"):
        del calls[:]
        scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route, read_filter=cfg, qc=qc)
        assert calls == [("before", ("cut a.fq",)), ("filter", ("cut a.fq",)), ("after", ("kept cut a.fq",)), (route,)]
        del calls[:]
        scan.scan_single_end_files("ref.fa", "x.csv", "a.fq", route=route)
        assert calls == [(route,)]


def test_the_streamed_routes_ask_for_the_full_cut_only_with_qc(monkeypatch):
    seen = []

    def source_stream(indexer, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((lean, kw))
        return iter(())
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    qc = _Qc()
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096)
    scan_stream.scan_pair_source_stream("ix", "r1", "r2", 4096, qc=qc)
    scan_stream.scan_single_text_stream("ix", "r1", 4096)
    scan_stream.scan_single_text_stream("ix", "r1", 4096, qc=qc)
    assert seen == [(None, {}), (False, {"qc": qc}), (None, {}), (None, {"qc": qc})]


class _B:
    """A batch of 5 records as far as ``_scan_chunk`` looks."""
    n_records, n_newlines = 5, 20

    def __init__(self, name, offsets=(0, 1, 2, 3, 4, 5)):
        self.name, self.offsets = name, list(offsets)

    def _replace(self, **kw):
        out = _B(self.name, kw["offsets"])
        out.n_records = kw["n_records"]
        return out


def test_a_chunk_measures_the_records_the_sides_share_not_the_batch(monkeypatch):
    """``_scan_chunk``: with ``qc`` the cut is the full one whatever ``lean`` says; the first m = 3 of a batch's 5
    records are measured before the filter and what the filter leaves behind it; the rest are the next chunk's."""
    from genefuserust_amd import fastq
    calls = []
    monkeypatch.setattr(fastq, "fastq_cut_device", lambda ix, t, lean=False: (calls.append(("cut", t, lean)), _B(t))[1])
    monkeypatch.setattr(scan_stream, "_record_cuts", lambda batches, texts, final, names: (3, [5] * len(texts), [0] * len(texts)))

    class _Totals:
        def cpu(self):
            return self

        def tolist(self):
            return [0] * 8

    def filter_chunk(ix, config, batches, m):
        calls.append(("filter", [b.name for b in batches], m))
        return [_B("kept " + b.name, b.offsets[:m + 1]) for b in batches], _Totals()
    monkeypatch.setattr(scan_stream, "_filter_chunk", filter_chunk)

    def scan_records(ix, texts, batches, m, done, max_read_len, names):
        calls.append(("scan", [b.name for b in batches]))
        return ("rec", b"", b"", [], {"pairs": m})
    qc = _Qc()
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, [(x.name, x.n_records, len(x.offsets)) for x in b]))
    args = ("ix", ["a", "b"], ["t1", "t2"], [False, False], 0, None, True, scan_records)
    _, _, (out, m, last) = scan_stream._scan_chunk(*args, read_filter=ReadFilter(), qc=qc)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("before", [("t1", 3, 4), ("t2", 3, 4)]),
                     ("filter", ["t1", "t2"], 3), ("after", [("kept t1", 3, 4), ("kept t2", 3, 4)]),
                     ("scan", ["kept t1", "kept t2"])]
    assert m == 3 and set(out[4]) == {"pairs"} | set(COUNTER_KEYS)   # the totals are the filter's alone
    # qc alone: the full cut, one measurement, today's scan and totals
    del calls[:]
    _, _, (out, _, _) = scan_stream._scan_chunk(*args, qc=qc)
    assert calls == [("cut", "t1", False), ("cut", "t2", False), ("before", [("t1", 3, 4), ("t2", 3, 4)]),
                     ("scan", ["t1", "t2"])] and out[4] == {"pairs": 3}
    # without: today's call, the lean cut for pairs, nothing measured
    del calls[:]
    scan_stream._scan_chunk(*args)
    assert calls == [("cut", "t1", True), ("cut", "t2", True), ("scan", ["t1", "t2"])]


def test_scan_report_hands_the_keyword_on_only_when_set(monkeypatch):
    seen = []
    monkeypatch.setattr(scan, "scan_pair_end_report", lambda *a, **k: (seen.append(("pair", k)), ([], {}))[1])
    monkeypatch.setattr(scan, "scan_single_end_report", lambda *a, **k: (seen.append(("single", k)), ([], {}))[1])
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", lambda *a, **k: (seen.append(("multi", k)), [])[1])
    qc = _Qc()
    for files in (("ref.fa", "x.csv", "r1.fq", "r2.fq"), ("ref.fa", "x.csv", "r1.fq"), ("ref.fa", "list.txt", "r1.fq", "r2.fq")):
        multi_csv_scan.scan_report(*files, qc=qc)
        multi_csv_scan.scan_report(*files)
    assert [w for w, _ in seen] == ["pair", "pair", "single", "single", "multi", "multi"]
    assert [k.get("qc", "absent") for _, k in seen] == [qc, "absent"] * 3


def test_multi_csv_measures_once_for_k_indexes(monkeypatch, tmp_path):
    """Streamed: the keyword goes to the one chunk loop, not to a loop over indexes.  Whole file: three CSVs, one
    measurement before the loop."""
    seen = []

    def source_stream(ix, sources, chunk_bytes, max_read_len, names, scan_records=None, lean=None, **kw):
        seen.append((ix, lean, kw))
        yield [("rec", b"", b"", [], dict(TOT, pairs=4))] * 3
    monkeypatch.setattr(scan_stream, "_scan_source_stream", source_stream)
    monkeypatch.setattr(scan_stream, "open_fastq_sources", lambda opened, files, inflate="host": list(files))
    import genefuserust_amd.fusion_mapper as fusion_mapper
    import genefuserust_amd.read_pair as read_pair
    monkeypatch.setattr(fusion_mapper, "FusionMapper", lambda ix: _Mapper())
    monkeypatch.setattr(read_pair, "finish_pair_hits", lambda *a: [])
    monkeypatch.setattr(scan, "named_from_device", lambda hits, rec, names, *orig: [])
    qc = _Qc()
    out = multi_csv_scan._stream_multi_csv(["ix0", "ix1", "ix2"], ("a.fq", "b.fq"), 4096, qc=qc)
    assert seen == [("ix0", False, {"qc": qc})] and len(out) == 3
    multi_csv_scan._stream_multi_csv(["ix0", "ix1", "ix2"], ("a.fq", "b.fq"), 4096)
    assert seen[-1] == ("ix0", False, {})
    # whole file
    calls = []

    class _Batch(str):
        def max_read_len(self):
            return 7

    class _Reader:
        def __init__(self, name):
            self.name = name

        def read_all_device(self, ix):
            return _Batch("cut " + self.name), b"text"
    from genefuserust_amd import fastq
    monkeypatch.setattr(fastq, "FastqReader", _Reader)
    monkeypatch.setattr(scan, "open_index", _open_index)
    monkeypatch.setattr(scan, "read_contigs", lambda ref: {})
    monkeypatch.setattr(scan, "single_end_found",
                        lambda *a: (calls.append(("scan",)), ([], *scan.route_counters("reads", 5, 0, TOT)))[1])
    monkeypatch.setattr(scan, "report_matches", lambda kept, counters, *a: ([], counters))
    lst = tmp_path / "panels.txt"
    for name in ("a.csv", "b.csv", "c.csv"):
        (tmp_path / name).write_text("")
    lst.write_text("".join("%s\n" % (tmp_path / name) for name in ("a.csv", "b.csv", "c.csv")))
    qc.measure = lambda ix, stage, *b, stream=None: calls.append((stage, b))
    got = multi_csv_scan.scan_multi_csv_report("ref.fa", str(lst), "r1.fq", qc=qc)
    assert len(got) == 3 and calls == [("before", ("cut r1.fq",)), ("scan",), ("scan",), ("scan",)]


# ---- the command line -------------------------------------------------------------------------------------------------

def test_the_command_line_options_reach_scan_report(monkeypatch, tmp_path, capsys):
    from genefuserust_amd import cli
    seen = []
    counters = dict(zip(COUNTER_KEYS, (9, 1, 2, 3, 4, 5, 6)), pairs=12)

    def scan_report(ref, fusion, r1, r2, **kw):
        seen.append(("one", kw))
        return ([], dict(counters)) if fusion.endswith(".csv") else [("a.csv", [], dict(counters)), ("b.csv", [], {})]

    def scan_multi_csv_report(ref, fusion, r1, r2, **kw):
        seen.append(("streamed list", kw))
        return [("a.csv", [], dict(counters)), ("b.csv", [], dict(counters))]
    monkeypatch.setattr(multi_csv_scan, "scan_report", scan_report)
    monkeypatch.setattr(multi_csv_scan, "scan_multi_csv_report", scan_multi_csv_report)
    for name in ("ref.fa", "x.csv", "panels.txt", "a.fq", "b.fq"):
        (tmp_path / name).write_text("")
    files = ["-1", str(tmp_path / "a.fq"), "-2", str(tmp_path / "b.fq"), "-r", str(tmp_path / "ref.fa"), "-h", "", "-j", ""]
    csv, lst = ["-f", str(tmp_path / "x.csv")], ["-f", str(tmp_path / "panels.txt")]
    out = tmp_path / "qc.json"
    assert cli.main(files + csv) == 0 and "qc" not in seen[-1][1] and not out.exists()   # off: the call of today
    assert cli.main(files + csv + ["--qc-json", str(out)]) == 0
    assert isinstance(seen[-1][1]["qc"], ReadQc) and seen[-1][1]["qc"].insert_size is True
    # nothing was measured by the stub: the document of an empty result, with the scan's counters
    empty = [np.zeros(model.SIDE_WORDS, dtype=np.int64)]
    assert out.read_text() == model.report_json(empty, empty, None, counters)
    assert json.loads(out.read_text())["filtering_result"]["passed_filter_reads"] == 9
    out.unlink()
    assert cli.main(files + csv + ["--qc-json", str(out), "--qc-no-insert-size"]) == 0
    assert seen[-1][1]["qc"].insert_size is False and out.exists()
    for mode, extra in (("one", []), ("streamed list", ["--chunk-bytes", "4096"])):   # a list of CSVs: one file, once
        out.unlink()
        assert cli.main(files + lst + extra + ["--qc-json", str(out)]) == 0 and seen[-1][0] == mode
        assert isinstance(seen[-1][1]["qc"], ReadQc)
        assert out.read_text() == model.report_json(empty, empty, None, counters)
        assert [p.name for p in tmp_path.iterdir() if p.name.startswith("qc")] == ["qc.json"]
    capsys.readouterr()
    count = len(seen)
    assert cli.main(files + csv + ["--qc-no-insert-size"]) == 1 and len(seen) == count
    assert "--qc-no-insert-size needs --qc-json" in capsys.readouterr().err


# ---- the document -----------------------------------------------------------------------------------------------------

def _hand_made():
    rng = np.random.default_rng(8)
    reads = lambda n, lo, hi: [(rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), L).tobytes(),   # noqa: E731
                                rng.integers(33, 75, L).astype(np.uint8).tobytes())
                               for L in rng.integers(lo, hi, n)]
    before = [model.stats_table(reads(40, 1, 90) + [(b"", b"")] * 3), model.stats_table(reads(43, 20, 600))]
    after = [model.stats_table(reads(30, 1, 60) + [(b"", b"")] * 13), model.stats_table(reads(20, 1, 50) + [(b"", b"")] * 23)]
    hist = np.zeros(model.INSERT_WORDS, dtype=np.int64)
    hist[[0, 30, 166, 170, 400, 1025]] = [7, 2, 11, 11, 3, 5]   # a tie: the smaller insert is the peak
    return before, after, hist


def test_report_json_against_the_model():
    before, after, hist = _hand_made()
    counters = dict(zip(COUNTER_KEYS, (50, 4, 44, 3, 2, 1, 6)), pairs=43, adapter_reads_cut=8, adapter_bases_cut=99,
                    adapter_cut_by_overlap=6, adapter_cut_by_sequence=2, adapter_overlapping_pairs=5)
    result = QcResult(tuple(before), tuple(after), hist)
    for c in (None, {"pairs": 43}, counters):
        assert read_qc.report_json(result, c) == model.report_json(before, after, hist, c)
    doc = json.loads(read_qc.report_json(result, counters))
    assert list(doc) == ["summary", "filtering_result", "adapter_cutting", "insert_size", "read1_before_filtering",
                         "read2_before_filtering", "read1_after_filtering", "read2_after_filtering"]
    assert list(doc["summary"]["before_filtering"]) == ["total_reads", "total_bases", "q20_bases", "q30_bases", "q20_rate",
                                                        "q30_rate", "read1_mean_length", "read2_mean_length", "gc_content"]
    assert doc["summary"]["before_filtering"]["total_reads"] == 83 and doc["summary"]["after_filtering"]["total_reads"] == 50
    assert doc["insert_size"]["peak"] == 166 and doc["insert_size"]["unknown"] == 12
    assert len(doc["insert_size"]["histogram"]) == 401 and doc["insert_size"]["histogram"][170] == 11
    r2 = doc["read2_before_filtering"]
    assert r2["total_cycles"] == 512 and len(r2["quality_curves"]["mean"]) == 512   # cut at 512: the tail row has no cycle
    assert list(r2["content_curves"]) == ["A", "T", "C", "G", "N", "GC"]
    r1 = doc["read1_after_filtering"]
    assert r1["total_cycles"] == len(r1["content_curves"]["GC"]) < 60
    for k in range(r1["total_cycles"]):
        assert abs(sum(r1["content_curves"][x][k] for x in "ATCGN") - 1.0) < 1e-12
    # single-end, no histogram: no read2, no insert_size
    single = QcResult((before[0],), (after[0],), None)
    doc = json.loads(read_qc.report_json(single))
    assert list(doc) == ["summary", "read1_before_filtering", "read1_after_filtering"]
    assert "read2_mean_length" not in doc["summary"]["before_filtering"]
    assert read_qc.report_json(single) == model.report_json(before[:1], after[:1])


def test_report_json_of_no_bases_and_no_inserts():
    """A rate over 0 bases is 0.0, a mean length over 0 reads 0, a peak of no insert 0."""
    zeros = np.zeros(model.SIDE_WORDS, dtype=np.int64)
    dropped = model.stats_table([(b"", b"")] * 4)
    hist = np.zeros(model.INSERT_WORDS, dtype=np.int64)
    hist[[0, 1025]] = [3, 1]
    result = QcResult((zeros, zeros), (dropped, dropped), hist)
    assert read_qc.report_json(result) == model.report_json([zeros, zeros], [dropped, dropped], hist)
    doc = json.loads(read_qc.report_json(result))
    for stage in ("before_filtering", "after_filtering"):
        assert doc["summary"][stage] == {"total_reads": 0, "total_bases": 0, "q20_bases": 0, "q30_bases": 0,
                                         "q20_rate": 0.0, "q30_rate": 0.0, "read1_mean_length": 0,
                                         "read2_mean_length": 0, "gc_content": 0.0}
    assert doc["insert_size"] == {"peak": 0, "unknown": 4, "histogram": [3]}
    assert doc["read1_after_filtering"] == {"total_cycles": 0, "quality_curves": {"mean": []},
                                            "content_curves": {k: [] for k in ("A", "T", "C", "G", "N", "GC")}}


def test_a_collector_that_measured_nothing():
    r = ReadQc().result()
    assert len(r.before) == len(r.after) == 1 and r.insert is None
    assert r.before[0].shape == (read_qc.SIDE_WORDS,) and not r.before[0].any() and not r.after[0].any()
    with pytest.raises(ValueError, match="stage"):
        ReadQc().measure("ix", "during", "batch")
    with pytest.raises(ValueError, match="stage"):
        r.summary("during")
